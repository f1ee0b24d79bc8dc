/*
 * gpsiq_rows.h -- the rows either side of the hot path, each bit-identical to the reference lines it
 * restates: the per-block host refresh batched (gps.c:2731-2765), the navigation message words (gps.c:617-884, 1008-1072,
 * 2066-2140) and the RINEX navigation readers (gps.c:1131-1891).  For run-ahead hosts that do not keep the reference's C host
 * model; a port of the reference that keeps it needs include/gpsiq.h only.  Same library (libgpsiq.so), host only.
 */
#ifndef GPSIQ_ROWS_H
#define GPSIQ_ROWS_H

#include "gpsiq.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- [next rows] per-block host refresh, batched ----------- */
/* What the reference does on the host just before every pass of the sample loop
 * (gps.c:2731-2765: computeRange -> computeCodePhase -> gain), for many 0.1 s blocks at
 * once.  Plain double-precision C on the host, same operation order as the reference, so
 * with the same libm the descriptors are identical; blocks are independent (each range
 * depends only on time and position; the Doppler of block k is the range difference to
 * block k-1), so the batch is spread over host threads.  Nav words are inputs
 * (the 30 s nav-message refresh, gps.c:2878-2885, stays with the caller). */
typedef struct gpsiq_ephem {       /* the ephem_t fields satpos()/computeRange() read (gps.h:155-196) */
    double toe_sec, toc_sec;       /* toe.sec, toc.sec */
    double m0, n, ecc, sqrta, sq1e2, A, aop, omg0, omgkdot, inc0, idot;
    double cuc, cus, cic, cis, crc, crs;
    double af0, af1, af2, tgd;
} gpsiq_ephem_t;

typedef struct gpsiq_iono {        /* ionoutc_t fields ionosphericDelay() reads (gps.h:198-206) */
    int32_t enable, vflg;
    double  alpha[4], beta[4];
} gpsiq_iono_t;

typedef struct gpsiq_track {       /* per-channel host state that persists between blocks */
    int32_t  prn;                  /* 1..32, <= 0 unused */
    int32_t  g0_week;  double g0_sec;      /* chan.g0: start of the nav-word buffer (gps.c:2045) */
    int32_t  rho0_week; double rho0_sec;   /* chan.rho0.g  */
    double   rho0_range;                   /* chan.rho0.range: pseudorange of the previous block (gps.c:2039) */
    double   carr_phase;                   /* initial carrier phase (gps.c:2208-2214) */
    uint32_t dwrd[GPSIQ_N_DWRD];
} gpsiq_track_t;

/* Initialise trk[i].rho0 and carr_phase at receiver time (week, sec) and position xyz the
 * way allocateChannel() does (gps.c:2199-2214).  prn, g0 and dwrd must be filled by the caller. */
int gpsiq_track_init(const gpsiq_ephem_t *eph, const gpsiq_iono_t *iono, int week, double sec,
                     const double xyz[3], gpsiq_track_t *trk, int nchan);

/* checkSatVisibility() (gps.c:2142-2162): geometric azimuth / elevation (radians, no light-time
 * correction) of one satellite from ECEF position xyz at receiver time (week, sec), and the test
 * elevation > elv_mask_deg.  Returns 1 visible, 0 not visible, negative on error; azel may be NULL.
 * (allocateChannel() itself always passes a mask of 0 degrees, gps.c:2175.) */
int gpsiq_sat_visibility(const gpsiq_ephem_t *eph, int week, double sec, const double xyz[3],
                         double elv_mask_deg, double azel[2]);

/* Blocks k = 0..nblocks-1 at receiver times t_k = incGpsTime^(k+1)(week, sec) (the reference
 * advances grx by 0.1 s before the first block, gps.c:2692, and after every block, gps.c:2932)
 * and positions xyz[k] (ECEF metres).  out is [nblocks][nchan]; trk is updated to the state
 * after the last block.  gain_x2 != 0 applies the Pluto factor (gps.c:2759-2763).
 * nthreads <= 0: one per online CPU. */
int gpsiq_refresh_batch(const gpsiq_ephem_t *eph, const gpsiq_iono_t *iono, int week, double sec,
                        const double *xyz, int nblocks, int nchan, int gain_x2,
                        gpsiq_track_t *trk, gpsiq_chan_t *out, int nthreads);

/* The same over several navigation-message epochs in ONE threaded pass (a run-ahead host refreshes the word
 * buffers every 30 s, gps.c:2878-2885, but the ranges -- the expensive part -- do not depend on them): epoch e
 * covers blocks [first_block[e], first_block[e+1]) (first_block[0] = 0, the last epoch ends at nblocks) and takes
 * dwrd / g0 from trk_epochs[e][c]; prn, rho0 and carr_phase come from trk_epochs[0], whose rho0 is updated to the
 * state after the last block.  Every epoch must hold the same satellites (one allocation per call). */
int gpsiq_refresh_epochs(const gpsiq_ephem_t *eph, const gpsiq_iono_t *iono, int week, double sec,
                         const double *xyz, int nblocks, int nchan, int gain_x2,
                         gpsiq_track_t *trk_epochs /* [nepochs][nchan] */, const int *first_block /* [nepochs] */,
                         int nepochs, gpsiq_chan_t *out, int nthreads);

/* gpsiq_refresh_epochs followed by gpsiq_quantize_batch(carry_in = NULL) in one pass over the blocks: the same
 * out[nblocks][nchan] gpsiq_qchan_t those two calls give (block 0 of a slot seeded from trk_epochs[0][c].carr_phase,
 * later blocks chained with the exact carrier prefix), without the double-precision descriptors -- 296 bytes per
 * channel and block, mostly the nav-word buffer -- ever being written to memory.  For a run-ahead host that feeds
 * gpsiq_set_descriptors / gpsiq_generate_quantized. */
int gpsiq_refresh_epochs_quantized(const gpsiq_ephem_t *eph, const gpsiq_iono_t *iono, int week, double sec,
                                   const double *xyz, int nblocks, int nchan, int gain_x2,
                                   gpsiq_track_t *trk_epochs /* [nepochs][nchan] */, const int *first_block /* [nepochs] */,
                                   int nepochs, double fs, int nsamp, gpsiq_qchan_t *out, int nthreads);

/* ---- [next rows] navigation message words ------------------- */
/* The 60-word rolling buffer dwrd[] the sample loop reads its data bits from
 * (gps.c:2811) is built by the reference from the broadcast ephemeris: eph2sbf()
 * (gps.c:617-884) packs 3 + 2*25 subframe pages, generateNavMsg() (gps.c:2066-2140) inserts
 * week number and TOW count, chains the (32,26) parity of computeChecksum() (gps.c:1008-1072)
 * from word to word and rolls the buffer by one 30 s frame.  Bit-exact restatements: */
#define GPSIQ_N_SBF_PAGE 53   /* gps.h:55: subframes 1-3 + 25 pages of subframes 4 and 5 */
#define GPSIQ_N_DWRD_SBF 10

typedef struct gpsiq_nav_eph {    /* the ephem_t fields eph2sbf() packs (gps.h:155-196) */
    int32_t toe_week, iode, iodc, reserved;
    double  toe_sec, toc_sec;
    double  deltan, cuc, cus, cic, cis, crc, crs, ecc, sqrta, m0, omg0, inc0, aop, omgdot, idot;
    double  af0, af1, af2, tgd;
} gpsiq_nav_eph_t;

typedef struct gpsiq_nav_utc {    /* ionoutc_t (gps.h:198-206) */
    int32_t vflg, dtls, tot, wnt;
    double  alpha[4], beta[4], A0, A1;
} gpsiq_nav_utc_t;

typedef struct gpsiq_nav_alm_sv { /* almanac_prn_t fields eph2sbf() reads (almanac.h:21-41) */
    uint32_t svid, valid;
    int32_t  toa_week, reserved;
    double   toa_sec, e, delta_i, omegadot, sqrta, omega0, aop, m0, af0, af1;
} gpsiq_nav_alm_sv_t;

typedef struct gpsiq_nav_state {  /* per channel: chan.dwrd, chan.ipage, chan.g0 */
    uint32_t dwrd[GPSIQ_N_DWRD];
    int32_t  ipage, g0_week;
    double   g0_sec;
} gpsiq_nav_state_t;

/* computeChecksum(): source bits 31..30 = D29*,D30* of the previous word, bits 29..6 = d1..d24.
 * nib != 0 solves d23,d24 so that D29 = D30 = 0 (words 2 and 10). */
uint32_t gpsiq_nav_parity(uint32_t source, int nib);
/* eph2sbf().  alm = 32 entries or NULL (--disable-almanac: every page-25/almanac slot empty). */
int gpsiq_nav_subframes(const gpsiq_nav_eph_t *eph, const gpsiq_nav_utc_t *utc,
                        const gpsiq_nav_alm_sv_t *alm,
                        uint32_t sbf[GPSIQ_N_SBF_PAGE][GPSIQ_N_DWRD_SBF]);
/* generateNavMsg(g = (week, sec), chan, init).  init != 0 at channel allocation (gps.c:2196),
 * 0 at every 30 s refresh (gps.c:2880-2885).  st->ipage selects the subframe 4/5 page and is advanced. */
int gpsiq_nav_message(const uint32_t sbf[GPSIQ_N_SBF_PAGE][GPSIQ_N_DWRD_SBF], int week, double sec,
                      int init, gpsiq_nav_state_t *st);

/* The 30 s refresh of every channel in one call (gps.c:2880-2885: generateNavMsg(grx, &chan[i], 0) for all allocated
 * channels): sbf is [nchan][GPSIQ_N_SBF_PAGE][GPSIQ_N_DWRD_SBF], st[nchan]. */
int gpsiq_nav_roll(const uint32_t *sbf, int nchan, int week, double sec, gpsiq_nav_state_t *st);

/* ---- [next rows] RINEX navigation files ---------------------- */
/* readRinex2() (gps.c:1131-1505) / readRinex3() (gps.c:1512-1891): fixed-column parse of a
 * GPS broadcast-ephemeris file (plain or gzip), records grouped into sets whenever the time
 * of clock advances by more than an hour, at most GPSIQ_EPHEM_SETS sets of 32 satellites. */
#define GPSIQ_EPHEM_SETS 13   /* gps.h:108 EPHEM_ARRAY_SIZE */
#define GPSIQ_MAX_SAT    32   /* gps.h:33 */

typedef struct gpsiq_rinex_eph {  /* one ephem_t (gps.h:155-196), in the groupings the other entry points take */
    int32_t vflg, sva, svh, code, flag;       /* validity, URA index, health (MSB set as the reference does), L2 code, L2P flag */
    int32_t t_y, t_m, t_d, t_hh, t_mm;        /* calendar time of clock */
    double  t_sec, fit;
    int32_t toc_week, reserved;
    gpsiq_ephem_t   orbit;                    /* what gpsiq_refresh_batch() takes (incl. working variables A, n, sq1e2, omgkdot) */
    gpsiq_nav_eph_t nav;                      /* what gpsiq_nav_subframes() takes */
} gpsiq_rinex_eph_t;

/* version: 2 or 3.  eph is [GPSIQ_EPHEM_SETS][GPSIQ_MAX_SAT]; utc receives the header's
 * ionosphere/UTC parameters (vflg set when all four header records were present, gps.c:1257-1259).
 * Returns the number of ephemeris sets (0 .. GPSIQ_EPHEM_SETS; the reference reports 14 for a file with more
 * than 13 hourly groups although it stores 13 -- the library does not), or the reference's error codes: -1 cannot open,
 * -2 wrong RINEX version for this reader, -3 not a GPS navigation file. */
int gpsiq_rinex_read(const char *path, int version, gpsiq_rinex_eph_t *eph, gpsiq_nav_utc_t *utc);
/* The set gps_thread_ep() would use for a start time (gps.c:2588-2608): first set with a
 * satellite whose toc is within one hour of (week, sec); -1 if none. */
int gpsiq_rinex_select(const gpsiq_rinex_eph_t *eph, int nsets, int week, double sec);

/* Receiver-noise sigma (gpsiq_set_noise, include/gpsiq.h) that puts a channel of this gain at C/N0 = cn0_dbhz dB-Hz at fs Hz:
 * the carrier table's amplitude is 250, so C = (250*gain)^2 and N0 = 2*sigma^2/fs, i.e. 250*|gain|*sqrt(fs / (2*10^(cn0/10))). */
double gpsiq_noise_sigma_for_cn0(double cn0_dbhz, double gain, double fs);

/* ---- Output level: scale, round and saturate in the kernels --------------------------------------------------------------
 * A gain in front of the quantiser and a quantiser that saturates, as every front end has.  Off by default, and with the level off
 * every output byte is what include/gpsiq.h states (the sums wrap, the int8 stream keeps bits 4..11).  With the level on, for each
 * sample and for I and Q alike:
 *     S   = the noiseless int16 element of the contract: (short)(sum over channels)                     (gps.c:2834)
 *     A   = S + z(n)                     plain integer, no wrap; z = 0 while the noise is off
 *     y   = floor((A * mult + 32768) / 65536)               exact integer arithmetic
 *     out = min(max(y, -qmax), qmax)
 * stored as int16 for GPSIQ_SC16 and as int8 for GPSIQ_SC08: there is no >> 4 in the int8 path, the level takes its place.  Unlike
 * the noise-only path, where the noise is added into the 16-bit sum and wraps with it, the noise is added after the signal sum
 * has been taken out, in 32 bits, so any sigma gpsiq_set_noise accepts is representable.  The clamp is symmetric: no DC offset.
 * qmax = 1 gives a 3-level stream, 7 a 4-bit one, 2047 a 12-bit DAC's range, each in the int8 / int16 container.
 * Ranges: 1 <= mult < 2^24; 1 <= qmax <= 32767, and <= 127 when a call renders GPSIQ_SC08 (checked by the rendering call, since the
 * format is its argument); otherwise GPSIQ_E_ARG.  Every drop-in call and gpsiq_launch honour it; gpsiq_generate_batch_multi uses
 * ctx[0]'s setting for every device.  Kernel variants without the stage return GPSIQ_E_STATE while it is on, as for the noise. */
typedef struct gpsiq_level {
    uint32_t mult;                 /* Q16: the scale is mult / 65536 */
    int32_t  qmax;                 /* symmetric clamp */
} gpsiq_level_t;
int gpsiq_set_level(gpsiq_ctx_t *ctx, const gpsiq_level_t *level);      /* NULL: off */
/* rms per component (I or Q) of nchan channels and noise of this sigma, in accumulator units: sqrt(sigma^2 + sum (250*gain)^2 / 2) */
double gpsiq_composite_rms(const double *gain, int nchan, double sigma);
/* the multiplier that takes rms_in to rms_out: rint(65536 * rms_out / rms_in), clamped to [1, 2^24 - 1] */
uint32_t gpsiq_level_mult(double rms_in, double rms_out);

/* ---- Despread: a device correlator that measures what a rendered stream holds ------------------------------------------------
 * The receiver's first stage -- wipe off carrier, code and data bit with the replica the descriptors define, integrate and dump --
 * over the resident descriptor set (gpsiq_set_descriptors) and a DEVICE stream laid out as gpsiq_launch writes it: block b at
 * src + (b - block0) * block_stride_bytes, interleaved I,Q, int8 for GPSIQ_SC08 and int16 for GPSIQ_SC16.  For every block, every
 * ACTIVE slot k in device order (the block's active channels counted from 0, the rule of gpsiq_patch_t.slot) and every segment j:
 *     (rI, rQ)(n) = what the closed form of include/gpsiq.h gives sample n for this channel alone with gain 1.0:
 *                   s*cosTable512[idx], s*sinTable512[idx]     (s = -1 where neg, idx = P(n) >> 50)
 *     sums[b][k][j].i = sum over n in segment j of  I(n)*rI(n) + Q(n)*rQ(n)
 *     sums[b][k][j].q = sum over n in segment j of  Q(n)*rI(n) - I(n)*rQ(n)
 * in exact int64 arithmetic; I(n), Q(n) are the stream's elements as stored (no << 4 for int8).  The data bit is part of neg: it is
 * wiped, a whole block sums coherently.  The gain is NOT part of the replica, so a channel rendered with gain 0 is a legitimate
 * noise-floor probe: it adds nothing to the stream and correlates like any other.  The replica is the closed form: patches of
 * GPSIQ_NCO_REFERENCE (gpsiq_set_patches) are not applied to it.
 * Segment j is samples [j*seg_len, min((j+1)*seg_len, nsamp)); nseg = ceil(nsamp / seg_len), and seg_len >= nsamp gives one segment
 * per block.  seg_len must be a multiple of 64 and at least 64 (else GPSIQ_E_ARG): nothing in the estimate below needs a 1 ms
 * boundary, and a row of 64 samples -- what one wave instruction of the kernels works on -- then lies in exactly one segment.
 * sums is [nblocks][nchan][nseg] with nchan the resident set's; prn[b][k] is the satellite of slot k; for k at or past the block's
 * active count prn is 0 and the sums are all zero.  stats (may be NULL) receives the stream's own statistics per block from the
 * same pass: sums and sums of squares of the I and of the Q elements, and clip_i / clip_q, the number of elements with |x| >= clip.
 * Bytes between the blocks (block_stride_bytes > 2*nsamp*sample_size) are never read.
 * The kernels are queued on hip_stream (a hipStream_t, NULL = the null stream), i.e. behind the caller's gpsiq_launch on that
 * stream; the call then waits, copies the results to the HOST arrays and returns: it is synchronous.  kernel_ms (may be NULL): the
 * kernel's device time.  Every call overwrites its outputs; the same call twice gives the same answer.  Errors as gpsiq_launch's:
 * GPSIQ_E_ARG for a bad argument, GPSIQ_E_STATE when the blocks are not resident.  (GPSIQ_DESPREAD_KERNEL=generic in the environment, read per call, takes the generic kernel where the row kernel would serve: the tests' cross-check;
 * GPSIQ_DESPREAD_TARGET_WGS=N sets the grid size below which the planner shortens the waves' runs, csrc/gpsiq_despread_plan.h.) */
typedef struct gpsiq_despread_sum { int64_t i, q; } gpsiq_despread_sum_t;
typedef struct gpsiq_block_stats {
    int64_t  sum_i, sum_q;
    uint64_t sumsq_i, sumsq_q;
    uint32_t clip_i, clip_q;
} gpsiq_block_stats_t;
int gpsiq_despread(gpsiq_ctx_t *ctx, int block0, int nblocks, int nsamp, int sample_size,
                   const void *src, size_t block_stride_bytes, void *hip_stream, int seg_len, int clip,
                   gpsiq_despread_sum_t *sums /* host [nblocks][nchan][nseg] */, uint8_t *prn /* host [nblocks][nchan] */,
                   gpsiq_block_stats_t *stats /* host [nblocks], may be NULL */, float *kernel_ms /* may be NULL */);
/* C/N0 of one channel from count >= 2 full-length segments of it (host arithmetic), with T = seg_len / fs:
 *     m = mean(i)      v = (sum (i - m)^2 / (count - 1) + sum q^2 / count) / 2      cn0 = 10 log10(m^2 / (2 v T))
 *     one_sigma_db = (10 / ln 10) * sqrt(1/count + 1/(count * T * 10^(cn0/10)))
 * (a channel of amplitude a = 250*gain in noise of sigma per component: m = seg_len * a * 250, v = seg_len * sigma^2 * 250^2, and
 * C/N0 = a^2 * fs / (2 sigma^2) = m^2 / (2 v T).)  GPSIQ_E_RANGE for count < 2, m <= 0 or v == 0. */
int gpsiq_cn0_estimate(const gpsiq_despread_sum_t *sums, int count, int seg_len, double fs,
                       double *cn0_dbhz, double *one_sigma_db);

/* ---- Packed streams: 4 and 2 bits per component, as narrow front ends and their players read them -----------------------------------
 * Two packed formats of the interleaved I,Q stream; both hold two's-complement fields with I in the low bits:
 *   GPSIQ_PK4   4 bits per component, one byte per complex sample:   byte n = (I(n) & 15) | ((Q(n) & 15) << 4)
 *               field range -7..7; the code of -8 is never produced
 *   GPSIQ_PK2   2 bits per component, two complex samples per byte:  byte m = nib(2m) | (nib(2m+1) << 4),
 *               nib(n) = (I(n) & 3) | ((Q(n) & 3) << 2); field range -1..1, the 3-level stream of qmax 1; for an odd nsamp the
 *               last byte's high nibble is 0
 * gpsiq_packed_block_bytes(nsamp, bits): nsamp for 4 bits, (nsamp + 1) / 2 for 2 bits (0 for nsamp <= 0 or another `bits`).
 *
 * gpsiq_pack packs a DEVICE stream laid out as gpsiq_launch writes it (block b at src_dev + b * src_stride, int8 for GPSIQ_SC08 and
 * int16 for GPSIQ_SC16; src_dev 4-byte aligned, the stride a multiple of 4) into device memory, block b at dst_dev + b * dst_stride
 * (dst_dev 4-byte aligned, dst_stride >= gpsiq_packed_block_bytes and a multiple of 4).  The packer SATURATES: an element outside the
 * field range is clamped to +-7 / +-1 (symmetric, like the output level's clamp: no DC), and such elements are COUNTED: *clipped
 * (may be NULL) is their number over the whole call, so a stream that was not levelled, or levelled for another format, packs to
 * something defined and the caller sees a non-zero count instead of a silent wrap.  Bytes past a block's packed length are never
 * written, source bytes past 2*nsamp*sample_size never read.  The ranges must not overlap (GPSIQ_E_ARG).  The kernel is queued on
 * hip_stream (a hipStream_t, NULL = the null stream), i.e. behind the caller's gpsiq_launch on that stream; the call then waits,
 * fetches the count and returns: synchronous, like gpsiq_despread.  kernel_ms (may be NULL): the kernel's device time.  nblocks == 0
 * or nsamp == 0 launches nothing and returns GPSIQ_OK with a count of 0.
 * gpsiq_unpack is the inverse: the fields sign-extended into int8 / int16 elements, no shift, exactly 2*nsamp elements per block --
 * what gpsiq_despread takes, so a packed stream can be measured.  unpack(pack(x)) is x clamped.
 *
 * gpsiq_generate_batch_packed is the run-ahead call (gpsiq_generate_batch, include/gpsiq.h) that delivers packed blocks to HOST
 * memory, pageable or page-locked, block b at dst_host + b * dst_block_stride (any stride >= gpsiq_packed_block_bytes).  ch is
 * [nblocks][nchan] in host memory.  It needs the output level on with qmax <= 7 for 4 bits and <= 1 for 2 bits, else GPSIQ_E_STATE:
 * the packer then clamps nothing and the bytes are exactly the levelled int8 stream's (a packer that did clamp: GPSIQ_E_DEVICE).  The call
 * works in pieces of about 32 MiB of rendered stream (GPSIQ_PACK_PIECE_BLOCKS=n in the environment, read per call: n blocks per piece):
 * gpsiq_generate_batch renders a piece into device staging of the context's, the packer packs it, and its rows cross to the host
 * while the next piece renders.  The result is byte for byte the pack of what ONE gpsiq_generate_batch call over the whole timeline
 * writes at GPSIQ_SC08, in both NCO models, with noise and with patches; carrier continuation, the noise block counter and
 * carr_phase_out are that call's.  When an inner call fails its error comes back as it is; dst_host is then undefined. */
#define GPSIQ_PK4 4
#define GPSIQ_PK2 2
size_t gpsiq_packed_block_bytes(int nsamp, int bits);
int gpsiq_pack(gpsiq_ctx_t *ctx, int nblocks, int nsamp, int sample_size,
               const void *src_dev, size_t src_stride, int bits,
               void *dst_dev, size_t dst_stride,
               void *hip_stream, uint64_t *clipped /* may be NULL */, float *kernel_ms /* may be NULL */);
int gpsiq_unpack(gpsiq_ctx_t *ctx, int nblocks, int nsamp, int bits,
                 const void *src_dev, size_t src_stride, int sample_size,
                 void *dst_dev, size_t dst_stride,
                 void *hip_stream, float *kernel_ms /* may be NULL */);
int gpsiq_generate_batch_packed(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch,
                                int nblocks, int nchan, int nsamp, double fs,
                                int bits, void *dst_host,
                                size_t dst_block_stride,
                                double *carr_phase_out /* [nchan], may be NULL */);

/* ---- Acquisition: a blind code-phase and Doppler search on the device -------------------------------------------------------------
 * What a receiver that knows nothing does first.  gpsiq_acquire searches ONE contiguous span of a DEVICE stream -- interleaved I,Q,
 * int8 for GPSIQ_SC08 and int16 for GPSIQ_SC16, elements as stored (no << 4 for int8), nsamp complex samples at src, the base 4-byte
 * aligned and no more, as gpsiq_launch leaves a block -- for a list of satellites over a grid of ndopp Doppler bins and nshift sample
 * shifts.  It needs no resident descriptors and no NCO mode; a stream from gpsiq_unpack is as good as any.  Every quantity up to the
 * power is an exact integer:
 *     ca[p][n]  = +1 where chip ((n * code_step) >> 56) % 1023 of satellite prn[p] (gpsiq_prn_code) is 0, -1 where it is 1 (the sign a
 *                 channel with data bit 0 is rendered with: include/gpsiq.h's neg), for n in [0, ncoh); n * code_step is the exact
 *                 product, code_step in units of 2^-56 chip per sample as gpsiq_qchan_t.code_step.  There is no data bit.
 *     carrier of bin d at absolute sample m (m = 0 at src):  idx = ((m * (carr_step0 + d * carr_step_inc)) mod 2^59) >> 50, the steps
 *                 in units of 2^-59 cycle per sample as gpsiq_qchan_t.carr_step (the sum and the product are integers; mod takes the
 *                 non-negative residue, so only the steps' residues mod 2^59 matter);
 *                 (rI, rQ) = (cosTable512[idx], sinTable512[idx]), the unit table gpsiq_despread uses (gain 1.0)
 *     yi(m) = I(m)*rI + Q(m)*rQ        yq(m) = Q(m)*rI - I(m)*rQ                       (gpsiq_despread's formulas and signs)
 *     for satellite p, bin d, shift s in [0, nshift) and dwell k in [0, nnoncoh):
 *     Xi = sum over n < ncoh of yi(s + k*hop + n) * ca[p][n]         Xq = the same sum with yq          both exact int64
 *     power[p][d][s], an IEEE double:  acc = 0.0; for k ascending:  acc = fl(acc + fl(fl(double(Xi)*double(Xi)) + fl(double(Xq)*double(Xq))))
 * with no fused multiply-add anywhere (|X| < 2^44: the conversions are exact), so that a sequential float64 loop gives the same bits.
 * Arguments: sample_size GPSIQ_SC08 or GPSIQ_SC16; ncoh a multiple of 64 with 64 <= ncoh <= 2^20; nshift >= 1, nnoncoh >= 1, hop >= 1;
 * 1 <= ndopp <= 1024; (nshift - 1) + (nnoncoh - 1)*hop + ncoh <= nsamp; 1 <= nprn <= 32 and every prn[p] in 1..32 (a satellite may be
 * listed twice); src not NULL and 4-byte aligned; prn and peaks not NULL: anything else is GPSIQ_E_ARG.  Bytes past
 * 2*nsamp*sample_size are never read (nor are samples at or past (nshift - 1) + (nnoncoh - 1)*hop + ncoh).
 * Outputs, all HOST memory:
 *     peaks[nprn][ndopp]     the maximum of power over s and the shift it is at, the lowest s on a tie; reserved is 0
 *     power (may be NULL)    the whole grid [nprn][ndopp][nshift], 8 bytes a cell
 *     corr  (may be NULL)    the X themselves, gpsiq_despread_sum_t [nprn][ndopp][nnoncoh][nshift]: 16 * nprn * ndopp * nnoncoh * nshift
 *                            bytes, also of device memory for the call -- for tests and small searches (32 satellites x 41 bins x 4
 *                            dwells x 2600 shifts: 218 MB)
 *     kernel_ms (may be NULL) the kernels' device time
 * The kernels are queued on hip_stream (a hipStream_t, NULL = the null stream), i.e. behind the caller's gpsiq_launch on that stream;
 * the call then waits, copies the results to the host arrays and returns: it is synchronous, like gpsiq_despread.  Every call
 * overwrites its outputs; the same call twice gives the same bytes.  src may also be page-locked host memory of gpsiq_host_alloc,
 * which the device reads in place (gpsiq_runahead --acquire searches one block so; far too slow for more than that).  (GPSIQ_ACQUIRE_KERNEL=generic in the environment, read per call,
 * takes the generic kernel where the matrix kernels would serve: the tests' cross-check; GPSIQ_ACQUIRE_KERNEL=mfma takes the matrix
 * kernels wherever they can serve, csrc/gpsiq_acquire_plan.h.) */
typedef struct gpsiq_acquire_peak {
    double  power;
    int32_t shift;
    int32_t reserved;
} gpsiq_acquire_peak_t;
int gpsiq_acquire(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, void *hip_stream,
                  const uint8_t *prn /* host [nprn] */, int nprn, uint64_t code_step, int64_t carr_step0, int64_t carr_step_inc, int ndopp,
                  int nshift, int ncoh, int nnoncoh, int hop,
                  gpsiq_acquire_peak_t *peaks /* host [nprn][ndopp] */, double *power /* host [nprn][ndopp][nshift], may be NULL */,
                  gpsiq_despread_sum_t *corr /* host [nprn][ndopp][nnoncoh][nshift], may be NULL */, float *kernel_ms /* may be NULL */);
/* The steps of a search at sample rate fs whose bins are f0_hz + d * df_hz (host arithmetic): rint(1.023e6 / fs * 2^56),
 * rint(f0_hz / fs * 2^59) and rint(df_hz / fs * 2^59).  GPSIQ_E_RANGE where gpsiq_qchan_t's ranges would be left: a code step of 0
 * or of 2^57 and more, |carr_step0| or |carr_step_inc| of 2^58 and more; GPSIQ_E_ARG for fs that is not positive and finite. */
int gpsiq_acquire_steps(double fs, double f0_hz, double df_hz, uint64_t *code_step, int64_t *carr_step0, int64_t *carr_step_inc);
/* The decision on one satellite's grid power[ndopp][nshift] (host arithmetic): *dopp, *shift the best cell (the lowest d, then the
 * lowest s, on a tie); *ratio the best cell divided by the largest cell, in any bin, whose shift is more than guard samples from the
 * best shift (|s - *shift| > guard, no wrap-around).  GPSIQ_E_RANGE if no such cell exists or that cell is 0; GPSIQ_E_ARG for a NULL
 * argument, ndopp < 1, nshift < 1 or guard < 0. */
int gpsiq_acquire_decide(const double *power, int ndopp, int nshift, int guard, int *dopp, int *shift, double *ratio);

/* ---- Follow: closed-loop code and carrier tracking on the device ---------------------------------------------------------------------
 * What a receiver does with what acquisition found: a delay-lock loop on the code, a frequency-then-phase lock loop on the carrier and
 * the prompt correlator the navigation bits come out of.  ("track" is the host channel state above; this stage is "follow".)
 * gpsiq_follow follows up to 32 satellites, independently of each other, through ONE contiguous span of a stream exactly as
 * gpsiq_acquire takes it: interleaved I,Q, int8 for GPSIQ_SC08 and int16 for GPSIQ_SC16, elements as stored, nsamp complex samples at
 * src, the base 4-byte aligned; device memory, or page-locked host memory of gpsiq_host_alloc.  No resident descriptors, no NCO mode.
 * Every quantity is an exact integer.  Below "/" on signed values is C's division of int64_t (it truncates toward zero), ">>" of a
 * negative value the arithmetic shift (it floors), and "X * 2^16" never leaves 63 bits (bounds in DESIGN.md 8f).
 *
 * State of one satellite, gpsiq_follow_state_t (filled by the caller, handed back so that a later call continues from it):
 *     prn         1..32
 *     sample      index into the span of the next epoch's first sample
 *     chip, code_frac   the prompt replica's code phase at `sample`: chip 0..1022 and a fraction in [0, 2^56), units of 2^-56 chip.
 *                 Never one word: 1023 * 2^56 does not fit 64 bits
 *     code_step0  the nominal code step (gpsiq_acquire_steps' value);  code_step  the current one; both in [2^52, 2^57)
 *     carr_phase  [0, 2^59), units of 2^-59 cycle;  carr_step  per sample, |carr_step| < 2^58
 *     carr_int    the loop's frequency integrator, units of carr_step, |carr_int| < 2^59
 *     prev_ip, prev_qp, have_prev   the previous epoch's scaled prompt (|.| <= 2^22) for the frequency discriminator
 *     epoch       epochs done so far: decides pull-in or phase lock
 *     status      written by the call, not read: 0 running (the launch limit is never seen by the caller), 1 the next epoch would pass the
 *                 end of the span, 2 the record array is full, 3 a step left its allowed range (also: code_step or carr_step outside
 *                 the range on entry, no record);  reserved comes back 0
 * A field outside the ranges above, other than code_step and carr_step, is GPSIQ_E_ARG.  From an acquisition peak at shift s of bin d:
 * sample = s, chip = 0, code_frac = 0, code_step = code_step0, carr_phase = 0, carr_step = carr_int = carr_step0 + d * carr_step_inc,
 * have_prev = 0, epoch = 0.  The decision-directed pull-in below has a false lock 500 Hz off; it pulls in from |error| < 250 Hz (a quarter
 * of the epoch rate), so a search that feeds the follower uses bins of 250 Hz or finer.
 *
 * One epoch is one period of the replica's code.  m = sample, c = code_step, w = carr_step, T0 = chip * 2^56 + code_frac (67 bits).
 *  1. N = ceil((1023 * 2^56 - T0) / c), the samples until the prompt replica enters the next period: 1 <= N <= 16368.  If m + N > nsamp
 *     the satellite stops with status 1; else if nepochs == max_epochs it stops with status 2.  Nothing is written for this epoch.
 *  2. For n in [0, N): idx = ((carr_phase + n*w) mod 2^59) >> 50, (rI, rQ) = (cosTable512[idx], sinTable512[idx]) (gpsiq_despread's unit
 *     table), yi = I*rI + Q*rQ, yq = Q*rI - I*rQ at sample m + n (gpsiq_despread's formulas and signs).  Taps t = early, prompt, late at
 *     off_t = +spacing, 0, -spacing (0 < spacing <= 2^56): A_t(n) = T0 + off_t + n*c, plus 1023 * 2^56 if T0 + off_t is negative;
 *     chip_t = (A_t(n) >> 56) mod 1023; ca_t(n) = +1 where that chip of gpsiq_prn_code(prn) is 0, -1 where it is 1 (acquire's sign).
 *     There is no data bit in the replica.
 *  3. Ie, Qe, Ip, Qp, Il, Ql = sum over n of yi * ca_t(n), yq * ca_t(n): exact int64.
 *  4. The record gpsiq_follow_epoch_t: sample, nsamp (= N), chip, code_frac, code_step, carr_phase, carr_step as they were at the start
 *     of the epoch, and the six sums; reserved 0.
 *  5. sh = max(0, bitlength(max |X| over the six sums) - 22), X' = X >> sh: every |X'| <= 2^22.
 *  6. Code: num = (Ie'-Il')*Ip' + (Qe'-Ql')*Qp', den = Ip'^2 + Qp'^2, ed = den ? (num * 2^16) / den : 0, clamped to [-2^16, 2^16].
 *     Positive: the replica is late, the code step rises.
 *  7. Carrier while epoch < pull_epochs (pull-in): w' = carr_int after, if have_prev,
 *         cross = prev_ip*Qp' - prev_qp*Ip', dot = prev_ip*Ip' + prev_qp*Qp'; if dot < 0, cross = -cross;
 *         ef = (|cross| + |dot|) ? (cross * 2^16) / (|cross| + |dot|) : 0;  carr_int += (ef * kf) >> 16.
 *  8. Carrier from epoch >= pull_epochs on (phase lock): numc = Ip' >= 0 ? Qp' : -Qp', denc = |Ip'| + |Qp'|,
 *         ec = denc ? (numc * 2^16) / denc : 0;  carr_int += (ec * ki) >> 16;  w' = carr_int + ((ec * kp) >> 16).
 *  9. carr_phase = (carr_phase + N*w) mod 2^59; total = code_frac + N*c, chip = chip + (total >> 56) - 1023, code_frac = total mod 2^56;
 *     sample += N; prev_ip, prev_qp = Ip', Qp'; have_prev = 1; epoch += 1.
 * 10. carr_step = w'; code_step = code_step0 + w' / 12320 + ((ed * kd) >> 16) (carrier aiding: 1540 cycles per chip, 2^59 / 2^56 = 8).
 *     If carr_step or code_step (as a signed sum, stored in 64 bits as it is) has left its range the satellite stops with status 3.
 *
 * gpsiq_follow_cfg_t: spacing in (0, 2^56]; pull_epochs >= 0; the gains kf, kp, ki, kd in [0, 2^46); reserved 0: else GPSIQ_E_ARG.
 * gpsiq_follow_gains fills it for sample rate fs (host arithmetic in double, then rint): with N0 = fs / 1000 and wn = pll_bn_hz / 0.53
 *     kf = fll_gain * 2^59 / (2 pi N0)       ki = wn^2 * 1e-3 / (2 pi) * 2^59 / fs       kp = 1.414 * wn / (2 pi) * 2^59 / fs
 *     kd = 4 * dll_bn_hz / (2 fs) * 2^56     spacing = 2^55     pull_epochs = 100
 * GPSIQ_E_ARG for an fs, gain or bandwidth that is not positive and finite, GPSIQ_E_RANGE where a gain leaves [0, 2^46).  The values the
 * tests and gpsiq_runahead use, (fs, 0.25, 18, 5), are tuned for strong signals.
 *
 * The call: state is host [nprn], in and out (1 <= nprn <= 32; a satellite may be listed twice); epochs is host [nprn][max_epochs]
 * (max_epochs >= 1), nepochs host [nprn]; kernel_ms (may be NULL) the kernels' device time.  A satellite runs until the span ends,
 * max_epochs records are written or a step leaves its range; state[p].status says which.  Records past nepochs[p] are not written.  It
 * is synchronous, like gpsiq_acquire, and queued on hip_stream behind the caller's work there.  The same call twice from the same input
 * state gives the same bytes; a call that stops on max_epochs and a second from the returned state give exactly the records and the
 * final state of one call -- a stream can be followed in pieces; a caller moving to a later span rebases state.sample itself.  Samples
 * at or past nsamp are never read.  (GPSIQ_FOLLOW_EPOCHS_PER_LAUNCH=n in the environment, read per call: the epochs one launch does per
 * satellite before the host relaunches from the device-resident state, csrc/gpsiq_follow_plan.h; the records do not depend on it.) */
typedef struct gpsiq_follow_state {
    uint64_t sample;
    uint64_t code_frac, code_step0, code_step;
    uint64_t carr_phase;
    int64_t  carr_step, carr_int;
    int64_t  prev_ip, prev_qp;
    uint32_t epoch;
    uint16_t chip;
    uint8_t  prn, have_prev;
    uint8_t  status;
    uint8_t  reserved[7];
} gpsiq_follow_state_t;
typedef struct gpsiq_follow_epoch {
    uint64_t sample;
    uint64_t code_frac, code_step;
    uint64_t carr_phase;
    int64_t  carr_step;
    int64_t  ie, qe, ip, qp, il, ql;
    uint32_t nsamp;
    uint16_t chip, reserved;
} gpsiq_follow_epoch_t;
typedef struct gpsiq_follow_cfg {
    uint64_t spacing;
    int32_t  pull_epochs, reserved;
    int64_t  kf, kp, ki, kd;
} gpsiq_follow_cfg_t;
#define GPSIQ_FOLLOW_RUNNING 0
#define GPSIQ_FOLLOW_SPAN_END 1
#define GPSIQ_FOLLOW_FULL 2
#define GPSIQ_FOLLOW_RANGE 3
int gpsiq_follow(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, void *hip_stream,
                 const gpsiq_follow_cfg_t *cfg,
                 gpsiq_follow_state_t *state /* host [nprn], in and out */, int nprn,
                 gpsiq_follow_epoch_t *epochs /* host [nprn][max_epochs] */, int max_epochs,
                 int *nepochs /* host [nprn] */, float *kernel_ms /* may be NULL */);
int gpsiq_follow_gains(double fs, double fll_gain, double pll_bn_hz, double dll_bn_hz, gpsiq_follow_cfg_t *cfg);
/* The navigation bits of one satellite's records (host, integer arithmetic).  Over the epochs from `skip` on it chooses *offset in 0..19
 * that maximises the sum over whole 20-epoch groups (group j: epochs skip + offset + 20 j .. + 19) of |sum of ip|, the lowest offset on a
 * tie; bits[j] is the sign of group j's sum (+1 or -1; 0 for a zero sum); *nbits the number of groups, of which the first max_bits are
 * written.  GPSIQ_E_RANGE with fewer than 40 epochs after skip; GPSIQ_E_ARG for a NULL argument, skip < 0 or max_bits < 0.  The polarity
 * of a Costas loop is ambiguous: the whole sequence may come out negated. */
int gpsiq_follow_bits(const gpsiq_follow_epoch_t *epochs, int nepochs, int skip,
                      int *offset, int8_t *bits, int max_bits, int *nbits);

/* ---- Filter: a device FIR stage that band-limits and decimates -------------------------------------------------------------------
 * The synthesiser samples rectangular chips at the output rate with unlimited bandwidth; a receiver behind a band-limited front end
 * sees the stream low-passed and, usually, at a lower rate.  gpsiq_filter is that front end as integers: a causal FIR with int16 taps
 * over ONE contiguous span, a decimator, a rounding shift and a symmetric clamp.  Integers only, like every other stage: a restatement
 * in numpy agrees with the device byte for byte.
 *
 * Input span.  src is ONE contiguous span of nsamp complex samples, interleaved I,Q, int8 for GPSIQ_SC08 and int16 for GPSIQ_SC16,
 * elements as stored, base 4-byte aligned -- the span gpsiq_acquire and gpsiq_follow take.  x(m) is sample m of src for 0 <= m < nsamp.
 * For -(ntaps-1) <= m < 0, x(m) is sample ntaps-1+m of head: ntaps-1 samples in the same format, 4-byte aligned; head == NULL means
 * those samples are zeros.
 * Output count.  Output j, 0 <= j < nout, sits at input index m_j = phase + j*decim.  nout = 0 if phase >= nsamp, otherwise
 * nout = (nsamp - phase + decim - 1) / decim; next_phase = phase + nout*decim - nsamp (gpsiq_filter_span: host arithmetic, either
 * result pointer may be NULL).
 * Arithmetic.  For I and Q alike: acc = sum over k < ntaps of taps[k] * x(m_j - k), exact and causal.  y = acc at shift == 0,
 * otherwise y = floor((acc + 2^(shift-1)) / 2^shift).  out = min(max(y, -qmax), qmax) with qmax 127 for an int8 dst and 32767 for an
 * int16 dst: the clamp is symmetric, like the output level's.  *clipped is the number of elements the clamp changed.
 * Ranges.  1 <= ntaps <= 512, 1 <= decim <= 16, 0 <= phase < decim, 0 <= shift <= 24, nsamp >= 0, both sample sizes GPSIQ_SC08 or
 * GPSIQ_SC16 in any of the four combinations: anything else is GPSIQ_E_ARG.  sum |taps[k]| <= 65535, else GPSIQ_E_RANGE: with it
 * |acc| < 2^31 for both input formats, so there is one accumulator width and no saturation rule inside the sum.
 * Memory.  dst is device memory, 4-byte aligned, and receives exactly nout complex samples back to back; bytes past them are never
 * written, bytes past 2*nsamp*sample_size of src never read.  dst must not overlap src or head (GPSIQ_E_ARG).  src, head and dst may
 * also be page-locked memory of gpsiq_host_alloc, as for gpsiq_acquire.  taps is host memory.
 * Stream order and return.  The taps cross to the device on hip_stream (a hipStream_t, NULL = the null stream) and the kernel is
 * queued there: it runs behind the caller's gpsiq_launch on that stream.  The call then waits, fetches the count and returns:
 * synchronous, like gpsiq_pack; taps may be overwritten once it has returned.  nsamp == 0 or nout == 0 launches nothing and returns
 * GPSIQ_OK with a count of 0.  *nout (may be NULL) is the output count; kernel_ms (may be NULL) the kernel's device time.  The same
 * call twice gives the same bytes.
 * Continuation is part of the contract: filtering a span in pieces gives exactly the bytes and the clip count of one call over the
 * whole span, when each piece is called with head set to the last ntaps-1 samples of the piece before (of the pieces before, where
 * one is shorter than that) and phase set to that piece's next_phase.
 *
 * gpsiq_filter_design is a Hamming-windowed sinc low-pass: h[k] = 2fc/fs * sinc(2fc/fs * (k - (ntaps-1)/2)) * (0.54 - 0.46 cos(2 pi
 * k/(ntaps-1))), normalised to sum 1, scaled by 2^shift and rounded with rint; the remainder that makes sum taps == 2^shift exactly is
 * added to the centre tap.  ntaps odd, 3 <= ntaps <= 511, 0 < cutoff_hz < fs/2, 8 <= shift <= 14 (GPSIQ_E_ARG).  The result is symmetric
 * with a DC gain of exactly 1 after the shift.  Double arithmetic: its properties are contract, its bits are not.
 *
 * gpsiq_generate_batch_filtered is gpsiq_generate_batch_packed's piece loop with the filter in the packer's place: a piece is rendered
 * into device staging at sample_size, filtered on a side stream and its rows cross to HOST memory (pageable or page-locked) while
 * the next piece renders.  It needs nsamp % decim == 0 (GPSIQ_E_ARG); output block b is nsamp/decim samples of out_sample_size at
 * dst_host + b*dst_block_stride.  The first block's history is zeros, phase is 0 throughout, and the ntaps-1 samples of history
 * cross from piece to piece inside the staging: the caller never sees them.  The result is byte for byte gpsiq_filter (head NULL,
 * phase 0) of what ONE gpsiq_generate_batch over the whole timeline writes, in both NCO models, with noise and level; carrier
 * continuation, the noise block counter and carr_phase_out are that call's.  ch is host memory only, as for the packed call.
 * GPSIQ_FILTER_PIECE_BLOCKS=n in the environment, read per call, sets the blocks per piece (default: about 32 MiB of rendered
 * stream); GPSIQ_FILTER_KERNEL=generic|mfma, read per call by both calls, forces a kernel where it can serve.  *clipped (may be NULL)
 * is the sum over the pieces. */
int gpsiq_filter(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, const void *head /* may be NULL */,
                 const int16_t *taps /* host [ntaps] */, int ntaps, int shift, int decim, int phase,
                 int out_sample_size, void *dst, void *hip_stream,
                 int *nout /* may be NULL */, uint64_t *clipped /* may be NULL */, float *kernel_ms /* may be NULL */);
int gpsiq_filter_span(int nsamp, int decim, int phase, int *nout, int *next_phase);          /* host arithmetic */
int gpsiq_filter_design(double fs, double cutoff_hz, int ntaps, int shift, int16_t *taps);   /* host arithmetic */
int gpsiq_generate_batch_filtered(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs,
                                  int sample_size, const int16_t *taps, int ntaps, int shift, int decim, int out_sample_size,
                                  void *dst_host, size_t dst_block_stride, uint64_t *clipped, double *carr_phase_out);

/* ---- Spectrum: the exact integer power spectrum of a device stream ------------------------------------------------------------------
 * The instrument that looks at a stream in the frequency domain: a Welch-style averaged periodogram of ONE span, a dense DFT over the
 * library's own carrier table, in integers end to end, so that a restatement in numpy agrees with the device bit for bit.
 *
 * Input.  src is ONE contiguous span of nsamp complex samples, interleaved I,Q, int8 for GPSIQ_SC08 and int16 for GPSIQ_SC16, elements
 * as stored, base 4-byte aligned and no more, in device memory or page-locked memory of gpsiq_host_alloc -- the span gpsiq_acquire,
 * gpsiq_follow and gpsiq_filter take.  No resident descriptors and no NCO mode are needed.
 * Segments.  N = nfft.  Segment q starts at sample q*hop; nseg = nsamp < N ? 0 : (nsamp - N)/hop + 1; ngroups = nseg / navg; group g is
 * segments g*navg .. g*navg + navg - 1.  Segments past the last whole group are not part of the result, and samples at or past
 * (ngroups*navg - 1)*hop + N are never read.  (gpsiq_spectrum_span: host arithmetic, either result pointer may be NULL.)
 * Arithmetic.  Everything is an exact integer.  c(i), s(i) are cosTable512[i & 511], sinTable512[i & 511], the unit table of
 * gpsiq_despread (amplitude 250; gpsiq_carrier_table of the plumbing reads it back), and T = 512 / N.  For segment q and bin k in
 * [0, N), with m = q*hop + n and idx = (k*n*T) mod 512:
 *     Xi[k] = sum over n < N of I(m)*c(idx) + Q(m)*s(idx)        Xq[k] = sum over n < N of Q(m)*c(idx) - I(m)*s(idx)
 * gpsiq_despread's formulas and signs: a tone turning at +k0*fs/N peaks in bin k0.  Window: GPSIQ_WINDOW_RECT is Y = X;
 * GPSIQ_WINDOW_HANN is Y[k] = 2*X[k] - X[(k-1) mod N] - X[(k+1) mod N], i and q separately: the Hann window applied across bins,
 * scaled by 4, exact because it is the definition.  Y' = Y >> shift on each component, an arithmetic shift that floors (Y' = Y at
 * shift 0).  power[g][k] = sum over the group's segments of Yi'^2 + Yq'^2, exact in uint64.  The sum does not depend on its order:
 * the device accumulates as it likes and the same call twice gives the same bytes.
 * Bound.  The sum can never wrap: with xmax 128 for int8 and 32768 for int16, W 1 for the rectangular window and 4 for Hann,
 * Ymax = W*N*500*xmax (|I c + Q s| <= 250 (|I| + |Q|)), Ys = Ymax at shift 0 and (Ymax >> shift) + 1 otherwise, a call needs
 * 2*navg*Ys^2 <= 2^64 - 1 (128-bit host arithmetic), else GPSIQ_E_RANGE.  gpsiq_spectrum_min_shift returns the smallest shift in
 * 0..40 that satisfies it (GPSIQ_E_RANGE if none does, GPSIQ_E_ARG for a bad argument): int8, N 512, Hann has Ymax = 2^17 * 1000 and
 * takes shift 0 up to navg 536 and shift 1 from 537.
 * Ranges.  nfft in {64, 128, 256, 512}; hop nfft/2 or nfft; window GPSIQ_WINDOW_RECT or GPSIQ_WINDOW_HANN; navg >= 1; 0 <= shift <= 40;
 * nsamp >= 0; sample_size GPSIQ_SC08 or GPSIQ_SC16; src not NULL and 4-byte aligned; power not NULL: anything else is GPSIQ_E_ARG.
 * With ngroups == 0 the call launches nothing, writes nothing to power and returns GPSIQ_OK with *ngroups = 0.
 * Stream order and return.  The kernels are queued on hip_stream (a hipStream_t, NULL = the null stream) behind the caller's work
 * there; the call then waits, copies power [ngroups][nfft] to the host and returns: synchronous, like gpsiq_acquire.  *ngroups (may be
 * NULL) is the group count, kernel_ms (may be NULL) the kernels' device time.  GPSIQ_SPECTRUM_KERNEL=generic|mfma in the environment,
 * read per call, forces a kernel where it can serve (the matrix kernel: int8 input); the bytes do not depend on it.
 *
 * gpsiq_spectrum_scale gives the factor that turns a cell of power into stream units squared per Hz, two-sided and complex:
 * 4^shift / (navg * 250^2 * G * N * fs), G = 1 for the rectangular window and 6 for Hann (as defined above w(n) = 2 - 2 cos(2 pi n/N)
 * and sum w^2 = 6N).  White noise of variance sigma^2 per component then reads 2 sigma^2 / fs in every bin.  Double arithmetic: its
 * value is contract to a relative 1e-12, its bits are not.  The table is a half-sample-offset sine, so every twiddle carries the same
 * rotation by pi/512, which drops out of the power; it is rounded, which puts a floor under the bins beside a strong one
 * (DESIGN.md 8h). */
#define GPSIQ_WINDOW_RECT 0
#define GPSIQ_WINDOW_HANN 1
int gpsiq_spectrum(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, void *hip_stream,
                   int nfft, int hop, int window, int navg, int shift,
                   uint64_t *power /* host [ngroups][nfft] */, int *ngroups /* may be NULL */, float *kernel_ms /* may be NULL */);
int gpsiq_spectrum_span(int nsamp, int nfft, int hop, int navg, int *nseg, int *ngroups);   /* host arithmetic */
int gpsiq_spectrum_min_shift(int sample_size, int nfft, int window, int navg);              /* host arithmetic: the shift, or a negative error */
int gpsiq_spectrum_scale(int nfft, int window, int navg, int shift, double fs, double *scale); /* host arithmetic */

/* ---- Mix: tones, chirps and delayed streams summed on the device -----------------------------------------------------------------------
 * The stage that puts something hostile or second-hand into a stream: a CW or swept jammer at a set J/S, a pulsed interferer, a
 * repeater (the stream again, delayed and turned in frequency), a second scenario.  One operation: a sum of up to GPSIQ_MIX_MAX_TERMS
 * terms onto an output stream, then the rounding shift and the counted symmetric clamp of the filter and the level stage.  Integers
 * only, like every other stage: a restatement in numpy agrees with the device byte for byte.
 *
 * Sample index.  For output sample n in [0, nsamp) the absolute index is m = m0 + n, a uint64 that wraps mod 2^64.
 * Terms.  terms is host memory, 1 <= nterms <= 8.  For term k:
 *   Gate.  on(m) = gate_period == 0 || (m + gate_offset) mod gate_period < gate_on (m + gate_offset wraps mod 2^64 first).  A term
 *   that is off contributes 0.
 *   Source sample (GPSIQ_MIX_STREAM, GPSIQ_MIX_ROTATED).  x(n) = 0 for n < skip, otherwise sample n - skip of src: interleaved I,Q, int8
 *   for sample_size GPSIQ_SC08 and int16 for GPSIQ_SC16, elements as stored.  Exactly max(0, nsamp - skip) samples of src are read; with
 *   skip >= nsamp nothing is.
 *   Sweep position.  r = m with sweep_period == 0, otherwise r = (m + sweep_offset) mod sweep_period (the sum wraps mod 2^64 first).
 *   Phase.  theta = (phase0 + m*step + tri(r)*rate) mod 2^59 in units of 2^-59 cycle, tri(r) = r(r-1)/2 the exact integer: the
 *   instantaneous step at sweep position r is step + r*rate.  Every product is taken mod 2^64, which is exact because 2^59 divides it.
 *   Table.  idx = theta >> 50, (c, s) = (cosTable512[idx], sinTable512[idx]): the unit table of gpsiq_despread, amplitude 250.
 *   Value.  GPSIQ_MIX_STREAM: t = (xi, xq).  GPSIQ_MIX_ROTATED: t = (xi*c - xq*s, xi*s + xq*c).  GPSIQ_MIX_TONE: t = (c, s).  A tone
 *   with a positive step peaks in the positive bin of gpsiq_spectrum.
 * Sum and output.  acc = sum over k of gain_k * t_k in int64, I and Q alike; it cannot wrap (|t| < 2^24, |gain| < 2^31, 8 terms).
 * y = acc at shift 0, otherwise y = floor((acc + 2^(shift-1)) / 2^shift); out = min(max(y, -qmax), qmax).  *clipped is the number of
 * elements the clamp changed.
 * Ranges.  1 <= nterms <= 8; 0 <= shift <= 40; 1 <= qmax <= 127 for an int8 dst (out_sample_size GPSIQ_SC08) and <= 32767 for an int16
 * dst; nsamp >= 0; kind one of the three; gate_on <= gate_period; sweep_offset < sweep_period where sweep_period != 0 and gate_offset <
 * gate_period where gate_period != 0 (0 otherwise); reserved fields 0; for the stream kinds src not NULL, 4-byte aligned, sample_size
 * GPSIQ_SC08 or GPSIQ_SC16; for a tone src NULL, skip 0; dst not NULL and 4-byte aligned: anything else is GPSIQ_E_ARG.
 * Memory.  dst and every src are device memory or page-locked memory of gpsiq_host_alloc.  dst may be THE SAME ADDRESS as a stream
 * term's src if that term has skip 0 and dst's sample size: the in-place case, a jammer added to a rendered stream where it lies.  Any
 * other overlap of dst with a range a term reads is GPSIQ_E_ARG.  Bytes past the ranges above are never read, bytes past
 * 2*nsamp*out_sample_size of dst never written.
 * Stream order and return.  The terms cross to the device on hip_stream (a hipStream_t, NULL = the null stream) and the kernel is
 * queued there, behind the caller's work; the call then waits, fetches the count and returns: synchronous, like gpsiq_filter.
 * nsamp == 0 launches nothing and returns GPSIQ_OK with a count of 0.  kernel_ms (may be NULL) is the kernel's device time.  The same
 * call twice gives the same bytes.  GPSIQ_MIX_KERNEL=generic|rows in the environment, read per call, forces a kernel where it can
 * serve; the bytes and the count do not depend on it.
 * Continuation is part of the contract: mixing a span in pieces gives exactly the bytes and the count of one call, when each later
 * piece is called with m0 advanced by the samples done and its terms advanced by gpsiq_mix_advance: for the stream kinds
 * skip' = max(0, skip - done) and src moves forward by max(0, done - skip) samples; everything else is untouched.
 *
 * gpsiq_mix_tone turns frequencies into the integers of a term: step = rint(f0/fs * 2^59); with sweep_s == 0 rate 0 and period 0,
 * otherwise period = rint(sweep_s*fs) and rate = rint((f1 - f0)/fs/period * 2^59): a sawtooth sweep from f0 to f1.  GPSIQ_E_RANGE where
 * |step| or |rate*period| reaches 2^58 (half the sampling rate), or the period is < 2 or >= 2^32; GPSIQ_E_ARG for an fs that is not
 * positive and finite, or a value that is not finite.
 * gpsiq_mix_gain gives gain = rint(amplitude * 2^shift / unit), unit 1 for GPSIQ_MIX_STREAM and 250 otherwise; GPSIQ_E_RANGE at
 * |gain| >= 2^31.  Units: a satellite of descriptor gain g has amplitude 250*g in an unlevelled stream and 250*g*mult/65536 with the
 * output level on (gpsiq_level_mult); a tone of amplitude A has power A^2; so J/S in dB is 20 log10(A / that amplitude).
 *
 * gpsiq_generate_batch_mixed is gpsiq_generate_batch_filtered's piece loop with the mixer in the filter's place: a piece is rendered
 * into device staging, mixed IN PLACE on a side stream -- a GPSIQ_MIX_STREAM term (base_gain, skip 0) plus the ntones tones (0..7,
 * GPSIQ_MIX_TONE only), at m0 + b0*nsamp for a piece that starts at block b0 -- and its rows cross to HOST memory while the next piece
 * renders.  The result is byte for byte, and count for count, gpsiq_mix of what ONE gpsiq_generate_batch over the whole timeline
 * writes, in both NCO models, with noise and level; carrier continuation, the noise block counter and carr_phase_out are that call's.
 * ch is host memory only, as for the filtered call.  GPSIQ_MIX_PIECE_BLOCKS=n in the environment, read per call, sets the blocks per
 * piece (default: about 32 MiB of rendered stream). */
#define GPSIQ_MIX_STREAM  0   /* t = x                       (unit 1)   */
#define GPSIQ_MIX_ROTATED 1   /* t = x * (c + j s)           (unit 250) */
#define GPSIQ_MIX_TONE    2   /* t = (c, s)                  (unit 250) */
#define GPSIQ_MIX_MAX_TERMS 8
typedef struct gpsiq_mix_term {
    int32_t  kind, sample_size;      /* sample_size: stream kinds, GPSIQ_SC08 / GPSIQ_SC16 */
    const void *src;                 /* stream kinds: sample 0 of the term; NULL for a tone */
    uint64_t skip;                   /* stream kinds: delay in samples, zeros before it */
    int32_t  gain, reserved;         /* signed integer gain; reserved 0 */
    uint64_t phase0;                 /* 2^-59 cycle, at absolute sample 0 */
    int64_t  step;                   /* 2^-59 cycle per sample */
    int64_t  rate;                   /* 2^-59 cycle per sample^2: the step grows by rate every sample */
    uint32_t sweep_period, sweep_offset;        /* 0: the sweep never restarts */
    uint32_t gate_period, gate_on, gate_offset, reserved2;   /* gate_period 0: always on */
} gpsiq_mix_term_t;
int gpsiq_mix(gpsiq_ctx_t *ctx, int nsamp, uint64_t m0, const gpsiq_mix_term_t *terms /* host */, int nterms,
              int shift, int qmax, int out_sample_size, void *dst, void *hip_stream,
              uint64_t *clipped /* may be NULL */, float *kernel_ms /* may be NULL */);
int gpsiq_mix_advance(gpsiq_mix_term_t *terms, int nterms, uint64_t done);                    /* host arithmetic */
int gpsiq_mix_tone(double fs, double f0_hz, double f1_hz, double sweep_s, int64_t *step, int64_t *rate,
                   uint32_t *sweep_period);                                                  /* host arithmetic */
int gpsiq_mix_gain(double amplitude, int kind, int shift, int32_t *gain);                    /* host arithmetic */
int gpsiq_generate_batch_mixed(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs, int sample_size,
                               int32_t base_gain, const gpsiq_mix_term_t *tones, int ntones /* 0..7, GPSIQ_MIX_TONE only */, uint64_t m0,
                               int shift, int qmax, void *dst_host, size_t dst_block_stride, uint64_t *clipped, double *carr_phase_out);

/* ---- Resample: a device polyphase resampler for rate and clock offset ------------------------------------------------------------------
 * The stage that takes a stream off the sample clock it was rendered on: one render feeds front ends at other rates (2.6 Msps to a
 * 2.048 Msps receiver), a stream that can no longer be rendered again (a jammer mixed in) changes rate, and a receiver whose clock is
 * off by some parts per million is a step slightly away from one.  gpsiq_filter decimates by whole numbers; this stage moves by any
 * ratio from 1/8 to 8, with a table of FIR rows indexed by the fraction of the output's position.  Integers only, like every other
 * stage: a restatement in numpy agrees with the device byte for byte.
 *
 * Input.  src is ONE contiguous span of nsamp complex samples, interleaved I,Q, int8 for GPSIQ_SC08 and int16 for GPSIQ_SC16, elements
 * as stored, base 4-byte aligned -- the filter's span.  x(m) is sample m of src for 0 <= m < nsamp.  For -(ntaps-1) <= m < 0, x(m) is
 * sample ntaps-1+m of head: ntaps-1 samples in the same format, 4-byte aligned; head == NULL means those samples are zeros.
 * Position.  pos0 and step are uint64_t in units of 2^-32 input sample.  Output j sits at p_j = pos0 + j*step, with integer index
 * m_j = p_j >> 32 and fraction f_j = p_j & 0xffffffff.  nout = 0 if pos0 >= nsamp * 2^32, otherwise nout = ceil((nsamp * 2^32 - pos0) /
 * step): every j with m_j < nsamp.  next_pos = pos0 + nout*step - nsamp * 2^32.  (gpsiq_resample_span: host arithmetic in 128 bits,
 * either result pointer may be NULL; its nsamp is 64 bits wide because the batch call spans more than an int, and must stay below
 * 2^60.)  nout can reach 2^34 when upsampling: it is 64 bits everywhere.
 * Taps.  taps is host memory, int16_t [nphases + 1][ntaps] with nphases = 2^log2_phases.  Row nphases is the caller's "phase 0, one
 * sample later"; it is read only when interp != 0, and it is always present.  With L = log2_phases: q_j = f_j >> (32 - L) (0 when
 * L == 0) and mu_j = interp ? (f_j >> (24 - L)) & 255 : 0 -- the eight bits of the fraction below the row index.
 * Arithmetic.  For I and Q alike: a0 = sum over k < ntaps of taps[q_j][k] * x(m_j - k), and with interp a1 = sum over k of
 * taps[q_j + 1][k] * x(m_j - k), both exact.  Without interp y = a0 at shift == 0, otherwise y = floor((a0 + 2^(shift-1)) / 2^shift).
 * With interp y = floor(((256 - mu_j) * a0 + mu_j * a1 + 2^(shift+7)) / 2^(shift+8)), evaluated in 64 bits.  out = min(max(y, -qmax),
 * qmax) with qmax 127 for an int8 dst and 32767 for an int16 dst.  *clipped is the number of elements the clamp changed.  The stage is
 * causal like the filter: the group delay is the taps' own, (ntaps-1)/2 input samples for the designed ones.
 * Ranges.  0 <= log2_phases <= 8, 1 <= ntaps <= 64, (nphases + 1) * ntaps <= 8256, 0 <= shift <= 16, interp 0 or 1,
 * 2^29 <= step <= 2^35 (a ratio from 1/8 to 8), pos0 < 2^63, nsamp >= 0, both sample sizes GPSIQ_SC08 or GPSIQ_SC16 in any of the four
 * combinations: anything else is GPSIQ_E_ARG.  Every one of the nphases + 1 rows must have sum over k of |taps[r][k]| <= 65535, else
 * GPSIQ_E_RANGE: with it |a0|, |a1| < 2^31 for both input formats, so there is one accumulator width; only the interpolated combine
 * needs 64 bits.
 * Memory.  dst is device memory, 4-byte aligned, and receives exactly nout complex samples back to back; bytes past them are never
 * written, bytes past 2*nsamp*sample_size of src never read.  dst must not overlap src or head (GPSIQ_E_ARG).  src, head and dst may
 * also be page-locked memory of gpsiq_host_alloc.  taps is host memory.
 * Stream order and return.  The taps cross to the device on hip_stream (a hipStream_t, NULL = the null stream) and the kernel is
 * queued there: it runs behind the caller's work on that stream.  The call then waits, fetches the count and returns: synchronous,
 * like gpsiq_filter; taps may be overwritten once it has returned.  nsamp == 0 or nout == 0 launches nothing and returns GPSIQ_OK with
 * a count of 0.  *nout, *next_pos, *clipped and *kernel_ms (the kernel's device time) may each be NULL.  The same call twice gives the
 * same bytes.  GPSIQ_RESAMPLE_KERNEL=generic|rows in the environment, read per call by both calls, forces a kernel; the bytes and the
 * count do not depend on it.
 * Continuation is part of the contract: resampling a span in pieces gives exactly the bytes, the count and the final next_pos of one
 * call over the whole span, when each piece is called with head set to the last ntaps-1 samples before it (of more than one earlier
 * piece, where a piece is shorter than that) and pos0 set to the previous piece's next_pos -- also where a piece is so short that it
 * yields no output (pos0 >= nsamp * 2^32: next_pos = pos0 - nsamp * 2^32).  A drifting clock is a step that changes between pieces:
 * that is why there is no in-call rate term.
 *
 * gpsiq_resample_step gives step = rint(2^32 * fs_in / (fs_out * (1 + ppb * 1e-9))): fs_out is the nominal rate of the receiver, ppb
 * how far its clock runs fast.  GPSIQ_E_RANGE outside the legal steps; GPSIQ_E_ARG for a rate that is not positive and finite, a ppb
 * that is not finite, or a NULL pointer.
 * gpsiq_resample_design fills taps [nphases + 1][ntaps] from a Hamming-windowed sinc prototype g with its cutoff at bandwidth * 0.5 *
 * min(1, 2^32/step) of the input rate, 0 < bandwidth <= 1: row r, tap k is g(k + r/nphases - (ntaps-1)/2), r = 0..nphases, with
 * g(t) = sinc(2 fc t) * (0.54 + 0.46 cos(2 pi t / (ntaps-1))) for |t| <= (ntaps-1)/2 and zero outside: the Hamming window of ntaps
 * points, centred like the sinc.  Row nphases therefore is row 0 shifted by one tap (taps[nphases][k] against taps[0][k+1]) with a zero
 * in the vacated last place, and every row between has its last tap zero.  Each row is scaled to a sum of 2^shift and rounded with
 * rint; the remainder goes to its largest tap (the first of equals), so every row sums to 2^shift exactly and the DC gain is 1 at every
 * phase.  Row 0 carries one end tap more than row nphases, so the two are scaled a little differently: they agree to that ratio, not to
 * the bit.  For 0 < r < nphases row nphases - r is row r mirrored, taps[nphases-r][k] == taps[r][ntaps-2-k], to the bit (the row
 * r = nphases/2 of an odd ntaps, whose two largest taps are equal, carries its remainder on the first of them).  8 <= shift <= 14,
 * 2 <= ntaps <= 64, the ranges above otherwise (GPSIQ_E_ARG); GPSIQ_E_RANGE if a row would break the bound on its sum of magnitudes.
 * Double arithmetic: its properties are contract, its bits are not.
 *
 * gpsiq_generate_batch_resampled is gpsiq_generate_batch_filtered's piece loop with the resampler in the filter's place: a piece is
 * rendered into one of two device staging buffers at sample_size, resampled on a side stream, and its samples cross to HOST memory
 * (pageable or page-locked) while the next piece renders; history and next_pos pass from piece to piece inside the call.  The output is
 * ONE contiguous stream of *nout samples of out_sample_size at dst_host, with no block structure, because the count per block varies.
 * Byte for byte, count for count and carr_phase_out bit for bit it equals gpsiq_resample, with head NULL, of what ONE
 * gpsiq_generate_batch over the whole timeline writes, in both NCO models, with noise and level.  dst_capacity (in samples) below
 * gpsiq_resample_span(nblocks*nsamp, pos0, step) is GPSIQ_E_ARG before anything is launched.  ch is host memory only, as for the
 * filtered call.  GPSIQ_RESAMPLE_PIECE_BLOCKS=n in the environment, read per call, sets the blocks per piece (default: about 32 MiB of
 * rendered stream).  *clipped (may be NULL) is the sum over the pieces. */
int gpsiq_resample(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, const void *head /* may be NULL */,
                   const int16_t *taps /* host [2^log2_phases + 1][ntaps] */, int log2_phases, int ntaps, int shift, int interp,
                   uint64_t step, uint64_t pos0, int out_sample_size, void *dst, void *hip_stream,
                   uint64_t *nout /* may be NULL */, uint64_t *next_pos /* may be NULL */, uint64_t *clipped /* may be NULL */,
                   float *kernel_ms /* may be NULL */);
int gpsiq_resample_span(uint64_t nsamp, uint64_t pos0, uint64_t step, uint64_t *nout, uint64_t *next_pos);     /* host arithmetic */
int gpsiq_resample_step(double fs_in, double fs_out, double ppb, uint64_t *step);                             /* host arithmetic */
int gpsiq_resample_design(uint64_t step, double bandwidth, int log2_phases, int ntaps, int shift, int16_t *taps);   /* host arithmetic */
int gpsiq_generate_batch_resampled(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs, int sample_size,
                                   const int16_t *taps, int log2_phases, int ntaps, int shift, int interp, uint64_t step, uint64_t pos0,
                                   int out_sample_size, void *dst_host, uint64_t dst_capacity /* samples */, uint64_t *nout,
                                   uint64_t *clipped, double *carr_phase_out);

/* ---- AGC: windowed device gain control, pulse blanker and requantiser -------------------------------------------------------------------
 * The stage between the analogue side and a narrow quantiser.  gpsiq_set_level and the shifts of the filter and the mixer are fixed
 * multipliers, right for the power the caller worked out beforehand; once gpsiq_mix adds a jammer or a pulsed interferer they are not.
 * This stage measures: the gain is feed-forward, constant over a window of W samples, and a pure function of exact integer power sums
 * of the windows before it; the blanker's threshold is absolute.  No sample-serial loop anywhere, integers only: a restatement in
 * numpy (tests/_agc_ref.py) agrees with the device byte for byte.
 *
 * Input.  src is ONE contiguous span of nsamp complex samples as gpsiq_filter takes it: interleaved I,Q, int8 for GPSIQ_SC08 and int16
 * for GPSIQ_SC16, elements as stored, base 4-byte aligned, device or page-locked memory.  dst receives exactly nsamp complex samples
 * of out_sample_size, in any of the four combinations.
 * Windows belong to the stream, not to the span.  The first W - state.fill samples of a span complete the window in progress;
 * nwin = ceil((fill + nsamp) / W) windows are touched and next_fill = (fill + nsamp) % W (gpsiq_agc_span: host arithmetic, either
 * result pointer may be NULL).  mults[i] is the multiplier of the i-th touched window.
 * Blanker.  exceed(m) holds iff blank_thresh > 0 and (|I(m)| > blank_thresh or |Q(m)| > blank_thresh), elements as stored.  blank(m)
 * holds iff m < state.hold, or exceed(e) holds for some e in [max(0, m - H), m], H = blank_hold.  Blanked samples are written as
 * (0, 0), counted in *blanked (in samples), and take no part in the power or in *clipped.  hold_out = max(0, hold_in - nsamp,
 * H - (nsamp - 1 - e_last)), the last term only where the span holds an exceeding sample, e_last the last one.
 * Power.  For a window, sum is the sum of I^2 + Q^2 over its unblanked samples and cnt is 2 per unblanked sample.  When a window
 * completes it enters the ring, which keeps the last M = navg.
 * Gain rule (exactly what gpsiq_agc_mult returns).  The multiplier of a window is fixed at the window's start, from S, the sum of wsum,
 * and n, the sum of wcnt, over the ring at that moment.  The ring does not change while a window is in progress, so a window continued
 * in the next call gets the same multiplier again.  n == 0 (which includes nring == 0): mult0.  Otherwise m = floor(S * 2^16 / n),
 * computed as ((S / n) << 16) + (((S % n) << 16) / n) -- the same value, inside 64 bits: S <= 2^53, n <= 2^23 --, r = max(isqrt(m), 1),
 * the floor square root: the rms in 1/256 units; mult = min(max(floor((target_q8 << 16) / r), mult_min), mult_max).
 * Output.  For I and Q alike y = floor((x * mult + 32768) / 65536) in 64 bits, the formula of the output level stage, and
 * out = min(max(y, -qmax), qmax).  *clipped counts the elements of unblanked samples that the clamp changed.
 * Ranges.  Those written at the members below; anything outside is GPSIQ_E_ARG, as is a state that cannot have come from a call with
 * this window and navg (nring > navg, fill >= window, pcnt > 2 * fill, hold > blank_hold), a NULL cfg, a pointer that is not 4-byte
 * aligned, and src and dst that overlap: there is no in-place form, the blanker reads input behind its output.  nsamp == 0 launches
 * nothing and returns GPSIQ_OK with counts of 0 and the state unchanged.  Entries of wsum / wcnt from nring on are zeros, in and out.
 * Stream order and return as gpsiq_filter's: all work is queued on hip_stream (a hipStream_t, NULL = the null stream) behind the
 * caller's producer there; the call then waits, fetches counts, multipliers and state, and returns.  The same call twice gives the
 * same bytes.  Bytes past 2 * nsamp * out_sample_size of dst are never written, bytes past the span never read; offsets are 64-bit.
 * Continuation is part of the contract: a span processed in pieces, each called with the state the piece before returned, gives
 * exactly what one call over the whole span gives -- the bytes, both counts, the concatenated multipliers (a window continued across
 * a call repeats its multiplier as the next call's mults[0]) and the final state.
 *
 * gpsiq_agc_mult(cfg, sumsq, count) is the gain rule on the host, for S = sumsq <= 2^53 and n = count <= 2^23.
 *
 * gpsiq_generate_batch_agc is the piece loop of the staged batch calls with this stage in the filter's place: a piece is rendered at
 * sample_size into one of two device staging buffers, taken through the stage on a side stream, and crosses to HOST memory (pageable
 * or page-locked) while the next piece renders.  The state stays on the device from piece to piece; it comes back once, behind the
 * last piece.  Output block b is nsamp samples of out_sample_size at dst_host + b * dst_block_stride.  Byte for byte, count for count,
 * state for state and carr_phase_out bit for bit it equals gpsiq_agc -- given the same state, or a fresh one -- of what ONE
 * gpsiq_generate_batch over the whole timeline writes, in both NCO models, with noise and level.  ch is host memory only.
 * GPSIQ_AGC_PIECE_BLOCKS=n in the environment, read per call, sets the blocks per piece (default: about 32 MiB of rendered stream). */
typedef struct gpsiq_agc_cfg {
    int32_t  window;      /* W: samples per gain window; a multiple of 64, 64..65536 */
    int32_t  navg;        /* M: complete windows the power is averaged over, 1..64 */
    uint32_t target_q8;   /* wanted rms per component of the output, in 1/256 output units; 1 .. 2^23-1 */
    uint32_t mult0;       /* Q16 multiplier while no window has completed, and for windows whose average holds no element */
    uint32_t mult_min, mult_max;   /* 1 <= mult_min <= mult_max < 2^24, and mult0 inside them */
    int32_t  blank_thresh;         /* 0: blanker off; else 1..32767, in input elements as stored */
    int32_t  blank_hold;           /* H: samples blanked behind an exceeding one, 0..1024 */
    int32_t  qmax;                 /* symmetric output clamp: 1..127 for an int8 dst, 1..32767 for int16 */
} gpsiq_agc_cfg_t;

typedef struct gpsiq_agc_state {   /* all zeros: a fresh stream */
    uint64_t wsum[64];  uint32_t wcnt[64];   /* the last nring complete windows, oldest first: sum of squares, elements counted */
    uint64_t psum;      uint32_t pcnt;       /* the window in progress */
    uint32_t fill;                           /* samples of it already seen, 0..W-1 */
    uint32_t nring;                          /* 0..M */
    uint32_t hold;                           /* samples at the start of the next span that are blanked whatever they hold, 0..H */
} gpsiq_agc_state_t;

int gpsiq_agc(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, const gpsiq_agc_cfg_t *cfg,
              gpsiq_agc_state_t *state /* host, in and out; NULL: fresh and not returned */,
              int out_sample_size, void *dst, void *hip_stream,
              uint32_t *mults /* host [nwin], may be NULL */, uint64_t *clipped, uint64_t *blanked, float *kernel_ms /* each may be NULL */);
int gpsiq_agc_mult(const gpsiq_agc_cfg_t *cfg, uint64_t sumsq, uint64_t count, uint32_t *mult);          /* host arithmetic: the gain rule */
int gpsiq_agc_span(uint64_t nsamp, int window, uint32_t fill, uint64_t *nwin, uint32_t *next_fill);      /* host arithmetic */
int gpsiq_generate_batch_agc(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs, int sample_size,
                             const gpsiq_agc_cfg_t *cfg, gpsiq_agc_state_t *state, int out_sample_size,
                             void *dst_host, size_t dst_block_stride, uint64_t *clipped, uint64_t *blanked, double *carr_phase_out);

/* ---- Complex filter and notch: a complex-tap device FIR, and the host arithmetic that turns a spectrum into a notch ------------------
 * gpsiq_filter has real taps, so its response is symmetric about 0 Hz: it cannot take a line out at +300 kHz and leave -300 kHz alone.
 * gpsiq_cfilter is the same stage with taps h[k] = re[k] + j im[k] over x(m) = I(m) + j Q(m):
 *   accI = sum over k < ntaps of re[k] * I(m_j - k) - im[k] * Q(m_j - k)
 *   accQ = sum over k < ntaps of re[k] * Q(m_j - k) + im[k] * I(m_j - k)
 * Everything else is gpsiq_filter's contract word for word (see "Filter"): the span, head and the zeros before it; the output count
 * and next_phase (gpsiq_filter_span serves both calls); y, the round-half-up shift, the symmetric clamp and *clipped; 1 <= ntaps <= 512,
 * 1 <= decim <= 16, 0 <= phase < decim, 0 <= shift <= 24, nsamp >= 0 and the four format pairs (GPSIQ_E_ARG); alignment and overlap
 * refusals; memory kinds; stream order and the synchronous return; nsamp == 0 or nout == 0 launching nothing; exact continuation
 * across pieces with head and next_phase.  The bound is sum over k of (|re[k]| + |im[k]|) <= 65535, else GPSIQ_E_RANGE: with it
 * |accI|, |accQ| <= 65535 * 32768 < 2^31 for both input formats, so there is one accumulator width and no saturation rule.
 * Two identities:  with every im[k] == 0 the call writes the bytes and the count of gpsiq_filter with taps = re;  with ntaps 1, re 0,
 * im 1, shift 0 it writes (-Q, I) (an element -32768 of an int16 stream becomes +32768 and is clamped to 32767, and counted).
 * GPSIQ_CFILTER_KERNEL=generic|mfma in the environment, read per call, forces a kernel where it can serve; the bytes and the count
 * never depend on it.
 *
 * gpsiq_notch_find reads ONE group of a gpsiq_spectrum result, power[nfft].  The floor is the median of the nfft cells: the lower of
 * the two middle ones, in integers.  A cell is over if power > ratio * floor (compared in long double).  A maximal run of over cells,
 * cyclic in k, is one line (at least half the cells are at or below the floor, so no run closes on itself).  Its frequency is the
 * power-weighted centroid of its cells, the run counted on from its first cell: bin k standing at (k < nfft/2 ? k : k - nfft) * fs/nfft and a run that wraps past bin nfft-1 continuing at nfft, nfft+1, ... before
 * the result is brought back into [-fs/2, fs/2); its excess is 10 log10(peak cell / floor).  Lines come back strongest first (by peak
 * cell, then by lower first bin), at most max_lines of them (1..8) in f_hz and excess_db; *nlines is what was found before that cap.
 * GPSIQ_E_ARG: nfft not one of 64, 128, 256, 512; ratio <= 1 or not finite; fs <= 0; max_lines outside 1..8; a floor of 0; a null pointer.
 *
 * gpsiq_notch_design writes the taps of a linear-phase notch at nlines frequencies.  ntaps odd, 3..511, c = (ntaps-1)/2.  g is the
 * Hamming-windowed sinc of gpsiq_filter_design at cutoff width_hz/2, normalised to sum 1 (unrounded).  The unrounded filter is
 *   h[n] = delta[n - c] - sum over l of a_l * g[n] * e^(j w_l (n - c)),   w_l = 2 pi f_l / fs,
 * where the a_l solve the nlines x nlines linear system that makes the unrounded response exactly 0 at every f_l (one line: a = 1), and
 * taps = rint(2^shift * h), component by component.  GPSIQ_E_ARG: ntaps even or outside 3..511, nlines outside 1..8, |f_l| >= fs/2,
 * width_hz outside (0, fs), two lines closer than width_hz (cyclically in fs), shift outside 8..14, a null pointer.  GPSIQ_E_RANGE:
 * the rounded taps break the sum bound or a component leaves int16; the caller then lowers shift.
 * Double arithmetic: its properties are contract, its bits are not.  With H the response of the integer taps over 2^shift:
 *   1. taps[c + n] = conj(taps[c - n]): linear phase, a delay of c samples;
 *   2. |H(f_l)| <= 0.7072 * ntaps / 2^shift: only rounding is left at a line, at most 0.5 per component and tap;
 *   3. where |f - f_l| >= width_hz/2 + 3.3 fs/ntaps for every l:  | |H(f)| - 1 | <= (sum |a_l|) * g_stop + 0.7072 * ntaps / 2^shift,
 *      g_stop the largest |G(f)| of the prototype g itself beyond that same distance from 0 Hz. */
typedef struct { int16_t re, im; } gpsiq_ctap_t;

int gpsiq_cfilter(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, const void *head /* may be NULL */,
                  const gpsiq_ctap_t *taps /* host [ntaps] */, int ntaps, int shift, int decim, int phase,
                  int out_sample_size, void *dst, void *hip_stream,
                  int *nout, uint64_t *clipped, float *kernel_ms);           /* the last three may be NULL */
int gpsiq_notch_find(const uint64_t *power /* [nfft], one group of gpsiq_spectrum */, int nfft, double fs, double ratio,
                     int max_lines, double *f_hz, double *excess_db, int *nlines);                    /* host arithmetic */
int gpsiq_notch_design(double fs, const double *f_hz, int nlines, double width_hz, int ntaps, int shift,
                       gpsiq_ctap_t *taps);                                                            /* host arithmetic */

/* ---- Array: covariance, weights and a combiner for several elements -------------------------------------------------------------------
 * Everything above reads ONE stream, and the notch can only take a narrowband line out.  Against a swept or broadband jammer a receiver
 * works in space: several antenna elements, the sample covariance of their streams, weights that put a null on the jammer, a combiner.
 * An element is the same timeline rendered with every channel's carr_phase advanced by the element's geometric phase (gpsiq_generate_batch
 * reads carr_phase where a slot is seeded or re-allocated, include/gpsiq.h) and with a noise seed of its own; a jammer from a direction is
 * a gpsiq_mix term whose phase0 differs per element.  nelem streams x_e(n) = I_e(n) + j Q_e(n), all of one sample_size, 1 <= nelem <=
 * GPSIQ_ARRAY_MAX_ELEM, given as a HOST array src[nelem] of stream pointers; every stream lies in device memory or in page-locked
 * memory from gpsiq_host_alloc, non-null where nsamp > 0 and 4-byte aligned; nsamp >= 0.  Anything else is GPSIQ_E_ARG.
 *
 * gpsiq_array_cov writes the exact covariance  R[a][b] = sum over n < nsamp of x_a(n) * conj(x_b(n))  to cov[a][b][0..1] (host, int64):
 *   Re R[a][b] = sum (Ia Ib + Qa Qb)        Im R[a][b] = sum (Qa Ib - Ia Qb)
 * The full matrix is written: the diagonal's imaginary part is exactly 0 and R[b][a] is the conjugate of R[a][b].  The sums cannot wrap:
 * one int16 term is at most 2 * 32768^2 = 2^31 in magnitude and nsamp < 2^31, so |R| < 2^62 (an int8 term is at most 2^15).  Everything
 * on the device is integers, and integer addition makes the order the workgroups' atomics arrive in irrelevant: the same call twice
 * gives the same numbers, whichever kernel serves.  nsamp == 0 launches nothing and writes zeros.  Stream order and return are
 * gpsiq_spectrum's: the call is queued on hip_stream behind the caller's work there, and returns synchronously.
 * GPSIQ_ARRAY_KERNEL=generic|mfma in the environment, read per call, forces a kernel where it can serve (the matrix kernel serves int8
 * input); the numbers never depend on it.
 *
 * gpsiq_array_combine is the beamformer  y(n) = sum over e of w_e * x_e(n),  w_e = re_e + j im_e:
 *   accI = sum over e of re_e * I_e(n) - im_e * Q_e(n)
 *   accQ = sum over e of re_e * Q_e(n) + im_e * I_e(n)
 * and each component goes through gpsiq_cfilter's finish: y = floor((acc + 2^(shift-1)) / 2^shift) (shift 0: acc), clamped to +-127 /
 * +-32767 of out_sample_size, *clipped the elements the clamp changed; 0 <= shift <= 24 and the four format pairs, else GPSIQ_E_ARG.
 * The bound is gpsiq_cfilter's: sum over e of (|re_e| + |im_e|) <= 65535, else GPSIQ_E_RANGE; with it |acc| <= 65535 * 32768 < 2^31 for
 * both input formats.  dst holds nsamp samples, 4-byte aligned, device or page-locked memory, and must not overlap any source
 * (GPSIQ_E_ARG).  nsamp == 0 launches nothing.  Stream order and return as above.  The operation is pointwise: a span combined in
 * pieces, each piece's sources and dst advanced alike, gives the bytes of one call and its counts add up to that call's count.
 * The two calls are tied by an identity: with shift 0 and nothing clamped,  sum |y(n)|^2 = sum over a, b of w_a conj(w_b) R[a][b]  exactly.
 *
 * gpsiq_array_steer: pos[e][0..2] is element e's position east, north, up in wavelengths; phase_cycles[e] = frac(pos_e . u) in [0, 1),
 * u = (cos el sin az, cos el cos az, sin el): the phase advance of a plane wave from that direction at the element.  GPSIQ_E_ARG: a
 * null pointer, nelem outside 1..8, a non-finite input.
 *
 * gpsiq_array_weights turns a covariance into the combiner's weights.  Rn = cov / nsamp + loading * (trace(cov / nsamp) / nelem) * I;
 * c = e_0 (steer_cycles NULL: power inversion, element 0 the reference) or c_e = exp(j 2 pi steer_cycles[e]) (minimum variance towards a
 * steering vector);  v = Rn^-1 c / (c^H Rn^-1 c), solved in long double through a Hermitian (Cholesky) factorisation written here;
 * w_e = rint(2^shift * conj(v_e)), component by component, so that the combiner's y = v^H x * 2^shift before its own shift.
 * GPSIQ_E_ARG: a null pointer, nelem outside 1..8, nsamp == 0, loading negative or not finite, a non-finite steering phase, shift outside
 * 0..24, a matrix that is not positive definite after loading.  GPSIQ_E_RANGE: a component leaves int16 or the rounded weights break the
 * sum bound; the caller then lowers shift.  Only the lower triangle of cov is read.
 * Long double arithmetic: its properties are contract, its bits are not.
 *   1. before rounding, v is the solution of Rn v = c / (c^H Rn^-1 c) to the accuracy the condition number of Rn leaves;
 *   2. | sum over e of w_e c_e - 2^shift | <= nelem / sqrt 2: only rounding is left in the constraint, at most 0.5 per component;
 *   3. v^H Rn v = 1 / (c^H Rn^-1 c) <= Rn[0][0] for power inversion (e_0 itself satisfies the constraint), and for Rn = s^2 I + J a a^H
 *      with a_0 of modulus 1 the residual jammer power J |v^H a|^2 is below s^2. */
#define GPSIQ_ARRAY_MAX_ELEM 8

int gpsiq_array_cov(gpsiq_ctx_t *ctx, int nelem, const void *const *src /* host [nelem] stream pointers */, int nsamp, int sample_size,
                    void *hip_stream, int64_t *cov /* host [nelem][nelem][2] */, float *kernel_ms /* may be NULL */);
int gpsiq_array_combine(gpsiq_ctx_t *ctx, int nelem, const void *const *src /* host [nelem] */, int nsamp, int sample_size,
                        const gpsiq_ctap_t *w /* host [nelem] */, int shift, int out_sample_size, void *dst, void *hip_stream,
                        uint64_t *clipped, float *kernel_ms);                /* the last two may be NULL */
int gpsiq_array_steer(const double *pos /* [nelem][3] */, int nelem, double az_rad, double el_rad, double *phase_cycles);   /* host arithmetic */
int gpsiq_array_weights(const int64_t *cov /* [nelem][nelem][2] */, int nelem, uint64_t nsamp, const double *steer_cycles /* may be NULL */,
                        double loading, int shift, gpsiq_ctap_t *w /* [nelem] */);                                         /* host arithmetic */

/* ---- Space-time array: covariance, weights and a combiner over elements and taps ------------------------------------------------------
 * Spatial weights have nelem - 1 degrees of freedom, and one reflection uses them up: a broadband jammer that reaches the elements
 * directly from one direction and again d samples later from another has a different spatial signature at every frequency, and two
 * elements cannot null it.  A tapped combiner can: W_0(z) = a_1 + b_1 z^-d, W_1(z) = -(a_0 + b_0 z^-d) is an exact null of
 * x_e = a_e j(n) + b_e j(n - d) with d + 1 taps.  These calls are the array's with a delay line behind every element.
 * Sizes: 1 <= nelem <= GPSIQ_ARRAY_MAX_ELEM, 1 <= ntaps <= GPSIQ_STAP_MAX_TAPS and K = nelem * ntaps <= GPSIQ_STAP_MAX_ROWS, else
 * GPSIQ_E_ARG.  Row k = e * ntaps + t of the space-time snapshot is  z_k(n) = x_e(n - t).
 * Samples before the span: for -(ntaps-1) <= m < 0, x_e(m) is sample ntaps-1+m of head[e]: ntaps-1 samples of the same format, 4-byte
 * aligned, in device or page-locked memory -- gpsiq_filter's head, one per element.  head == NULL or head[e] == NULL: zeros.  head is a
 * HOST array [nelem]; with ntaps == 1 it is not read.  Sources: as gpsiq_array_* has them (see "Array").
 *
 * gpsiq_stap_cov writes the exact covariance  R[k][l] = sum over 0 <= n < nsamp of z_k(n) * conj(z_l(n))  to cov[k][l][0..1] (host,
 * int64), real and imaginary parts as gpsiq_array_cov states them.  The full Hermitian matrix is written; the wrap bound is the
 * array's (|R| < 2^62); nsamp == 0 launches nothing and writes zeros.  Continuation: a span taken in pieces, each piece given head =
 * the last ntaps-1 samples before it (the first piece the span's own head), gives covariances that add up to one call's, word for word.
 * GPSIQ_STAP_KERNEL=generic|mfma in the environment, read per call, forces a kernel where it can serve (the matrix kernel serves int8
 * input); the numbers never depend on it.  Stream order and return: as gpsiq_array_cov.
 *
 * gpsiq_stap_combine is the tapped beamformer  y(n) = sum over e, t of w[e][t] * x_e(n - t),  w = re + j im:
 *   accI = sum over e, t of re[e][t] * I_e(n - t) - im[e][t] * Q_e(n - t)
 *   accQ = sum over e, t of re[e][t] * Q_e(n - t) + im[e][t] * I_e(n - t)
 * and each component goes through gpsiq_cfilter's finish (round-half-up shift, symmetric clamp, *clipped); 0 <= shift <= 24 and the
 * four format pairs, else GPSIQ_E_ARG.  The bound: sum over all K weights of (|re| + |im|) <= 65535, else GPSIQ_E_RANGE; with it
 * |acc| < 2^31 for both input formats.  dst holds nsamp samples, 4-byte aligned, device or page-locked memory, and overlaps no source
 * and no head (GPSIQ_E_ARG).  nsamp == 0 launches nothing.  Pieces with heads, sources and dst advanced alike, give the bytes of one
 * call, and their counts add up to its count.  Stream order and return: as gpsiq_array_combine.
 * Identities:  with ntaps == 1 both calls give the words and bytes of gpsiq_array_cov and gpsiq_array_combine;  the sub-matrix of the
 * rows with t == 0 is gpsiq_array_cov's result whatever head holds;  with nelem == 1 gpsiq_stap_combine writes the bytes and the count
 * of gpsiq_cfilter with taps = w[0], decim 1, phase 0 and the same head;  with shift 0 and nothing clamped,
 * sum |y(n)|^2 = sum over k, l of w_k conj(w_l) R[k][l]  exactly.
 *
 * gpsiq_stap_weights is gpsiq_array_weights over the K rows, through the same long double Cholesky factorisation:
 * Rn = cov / nsamp + loading * (trace(cov / nsamp) / K) * I;  the constraint is  c_(e,t) = [t == ref_tap] * (steer_cycles ?
 * exp(j 2 pi steer_cycles[e]) : [e == 0]);  v = Rn^-1 c / (c^H Rn^-1 c);  w[e][t] = rint(2^shift * conj(v_(e,t))).  Refusals as
 * gpsiq_array_weights (with the sizes above), and ref_tap outside 0..ntaps-1 is GPSIQ_E_ARG.  Only the lower triangle of cov is read.
 * Properties are contract, bits are not: the three of gpsiq_array_weights hold with K for nelem in property 2 and, in property 3, the
 * diagonal entry of row (0, ref_tap) for Rn[0][0]: v^H Rn v <= Rn[ref_tap][ref_tap] for power inversion, that row itself meeting the
 * constraint; and
 *   4. for the same covariance, v^H Rn v is at most that of the spatial solution (gpsiq_array_weights with the same loaded matrix) on
 *      the sub-matrix of the rows with t == ref_tap: a subspace cannot do better. */
#define GPSIQ_STAP_MAX_TAPS 8
#define GPSIQ_STAP_MAX_ROWS 32          /* nelem * ntaps */

int gpsiq_stap_cov(gpsiq_ctx_t *ctx, int nelem, const void *const *src /* host [nelem] stream pointers */,
                   const void *const *head /* host [nelem], may be NULL, entries may be NULL */, int nsamp, int sample_size, int ntaps,
                   void *hip_stream, int64_t *cov /* host [K][K][2] */, float *kernel_ms /* may be NULL */);
int gpsiq_stap_combine(gpsiq_ctx_t *ctx, int nelem, const void *const *src /* host [nelem] */, const void *const *head /* as above */,
                       int nsamp, int sample_size, const gpsiq_ctap_t *w /* host [nelem][ntaps] */, int ntaps, int shift,
                       int out_sample_size, void *dst, void *hip_stream, uint64_t *clipped, float *kernel_ms);   /* the last two may be NULL */
int gpsiq_stap_weights(const int64_t *cov /* [K][K][2] */, int nelem, int ntaps, uint64_t nsamp, const double *steer_cycles /* [nelem] or NULL */,
                       int ref_tap, double loading, int shift, gpsiq_ctap_t *w /* [nelem][ntaps] */);             /* host arithmetic */

/* Several beams from one pass.  A steered beam protects the one satellite it is steered at, so a receiver forms one beam per satellite
 * in view: 1 <= nbeams <= GPSIQ_STAP_MAX_BEAMS beams of the same sources, heads, ntaps, shift and formats, the element streams read
 * once.  w is [nbeams][nelem][ntaps], dst a HOST array [nbeams] of stream pointers, clipped a host array [nbeams] (may be NULL).
 *
 * gpsiq_stap_beams: for every beam b, dst[b] receives exactly the bytes gpsiq_stap_combine writes with w[b] and the same sources,
 * heads, ntaps, shift and formats, and clipped[b] is that call's count.  Rows, heads, the finish (round-half-up shift, symmetric
 * clamp), 0 <= shift <= 24 and the four format pairs are gpsiq_stap_combine's, and so are its refusals; nbeams outside 1 ..
 * GPSIQ_STAP_MAX_BEAMS is GPSIQ_E_ARG.  The bound holds per beam: sum over the K weights of beam b of (|re| + |im|) <= 65535, else
 * GPSIQ_E_RANGE.  Every dst[b] is non-null where nsamp > 0, 4-byte aligned, in device or page-locked memory, and overlaps no source,
 * no head and no other destination, else GPSIQ_E_ARG.  nsamp == 0 launches nothing and writes zero counts.  Pieces with heads, sources
 * and every dst advanced alike give the bytes of one call, and their counts add up per beam.  Stream order and return: as
 * gpsiq_stap_combine.  GPSIQ_STAP_BEAMS_KERNEL=generic|mfma in the environment, read per call, forces a kernel where it can serve (the
 * matrix kernel serves both input formats where nelem times ntaps rounded up to a power of two does not pass GPSIQ_STAP_MAX_ROWS and
 * every weight component lies in -32639 .. 32639, re also down to -32768); the bytes never depend on it.
 *
 * gpsiq_stap_beam_weights: beam b is what gpsiq_stap_weights returns for steer_cycles[b] (non-null: [nbeams][nelem]) with the same
 * remaining arguments, bit for bit.  The beams are solved in order; the first beam that is refused decides the return value, and
 * nothing is written for that beam or any beam after it.  nbeams outside 1 .. GPSIQ_STAP_MAX_BEAMS is GPSIQ_E_ARG. */
#define GPSIQ_STAP_MAX_BEAMS 8

int gpsiq_stap_beams(gpsiq_ctx_t *ctx, int nelem, const void *const *src /* host [nelem] */,
                     const void *const *head /* host [nelem], may be NULL, entries may be NULL */,
                     int nsamp, int sample_size,
                     const gpsiq_ctap_t *w /* host [nbeams][nelem][ntaps] */, int ntaps, int nbeams, int shift,
                     int out_sample_size, void *const *dst /* host [nbeams] stream pointers */, void *hip_stream,
                     uint64_t *clipped /* host [nbeams], may be NULL */, float *kernel_ms /* may be NULL */);
int gpsiq_stap_beam_weights(const int64_t *cov /* [K][K][2] */, int nelem, int ntaps, uint64_t nsamp,
                            const double *steer_cycles /* [nbeams][nelem] */, int nbeams, int ref_tap,
                            double loading, int shift, gpsiq_ctap_t *w /* [nbeams][nelem][ntaps] */);   /* host arithmetic */

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
