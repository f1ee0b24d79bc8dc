// gpsiq_follow_kernels.hip -- gfx950 (MI355X, wave64) kernel of gpsiq_follow (include/gpsiq_rows.h, "Follow"): a delay-lock loop on the
// code and a frequency-then-phase lock loop on the carrier, closed on the device.  Every quantity is an integer, so records and states
// are a pure function of (arguments, stream bytes).
// The loop is serial in time per satellite: what epoch e + 1 correlates against is decided by epoch e's sums.  One workgroup of four
// waves serves one satellite and loops over its epochs inside the kernel:
//   the state thread (thread 0) holds gpsiq_follow_state_t in registers.  At the top of an epoch it decides whether there is one
//       (steps in range, the epoch inside the span, room for its record) and hands its length, first sample, steps and the three taps'
//       code phases to the waves through LDS, together with the decision itself;
//   every wave takes every fourth row of 64 samples, a lane one sample of a row (masked at the ragged tail): one load, one look-up of
//       the unit carrier table, three of the code, six sums.  The products stay below 2^24 and go into int64 lane sums;
//   the lane sums are reduced with __shfl_xor inside a wave and through LDS across the waves;
//   the state thread runs steps 5 to 10 of the contract in scalar integer code and stores the record.
// No workgroup waits for another: no grid barrier, no flag, no spinning.  The decision to leave the epoch loop is the state thread's
// and is read by every thread from LDS behind a barrier, so every wave takes every barrier the same number of times.  A launch does at
// most per_launch epochs per satellite (gpsiq_follow_plan.h); the host relaunches from the states left in device memory.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_follow_geometry.h"
#include "gpsiq_signal.h"

namespace gpsiq {
namespace {

constexpr int64_t kFollowCodeMin = INT64_C(1) << 52, kFollowCodeEnd = INT64_C(1) << (GPSIQ_CODE_FRAC_BITS + 1);
constexpr int64_t kFollowCarrEnd = INT64_C(1) << (GPSIQ_CARR_FRAC_BITS - 1);

// what the state thread hands the waves for one epoch
struct FollowEpoch {
    uint64_t m, c, w, phase;       // first sample, code step, carrier step (mod 2^64), carrier phase
    uint64_t frac[3];              // early, prompt, late: the tap's code phase at the epoch's first sample,
    uint32_t chip[3];              // as a chip in [0, 1023] and a 56-bit fraction
    uint32_t N;
    int      go;                   // 0: the satellite has stopped, or the launch has done its share
};

// N = ceil(((1023 - chip) * 2^56 - frac) / c), 1 <= N <= 16368 for c in [2^52, 2^57).  The quotient is estimated in double (far
// better than to one unit: it is below 2^14) and settled with exact 128-bit products, whatever the estimate.
__device__ __forceinline__ uint32_t follow_len(uint32_t chip, uint64_t frac, uint64_t c)
{
    const unsigned __int128 R = ((unsigned __int128) (GPSIQ_CA_SEQ_LEN - chip) << GPSIQ_CODE_FRAC_BITS) - (unsigned __int128) frac;
    const double r = (double) (uint64_t) (R >> 64) * 18446744073709551616.0 + (double) (uint64_t) R;
    uint64_t q = (uint64_t) (r / (double) c);
    while ((unsigned __int128) q * (unsigned __int128) c < R) ++q;
    while (q > 0 && (unsigned __int128) (q - 1) * (unsigned __int128) c >= R) --q;
    return (uint32_t) q;
}

__device__ __forceinline__ int64_t follow_abs(int64_t x) { return x < 0 ? -x : x; }

// steps 4 to 10 of the contract: the record, the discriminators, the advance and the next steps
__device__ __forceinline__ void follow_close(gpsiq_follow_state_t &st, const gpsiq_follow_cfg_t &cfg, uint32_t N, const int64_t X[kFollowSums],
                                             gpsiq_follow_epoch_t *__restrict__ rec)
{
    rec->sample = st.sample; rec->code_frac = st.code_frac; rec->code_step = st.code_step; rec->carr_phase = st.carr_phase;
    rec->carr_step = st.carr_step;
    rec->ie = X[0]; rec->qe = X[1]; rec->ip = X[2]; rec->qp = X[3]; rec->il = X[4]; rec->ql = X[5];
    rec->nsamp = N; rec->chip = st.chip; rec->reserved = 0;

    uint64_t top = 0;
    for (int i = 0; i < kFollowSums; ++i) { const uint64_t a = (uint64_t) follow_abs(X[i]); top = a > top ? a : top; }
    const int len = top ? 64 - __clzll((long long) top) : 0, sh = len > 22 ? len - 22 : 0;
    const int64_t ie = X[0] >> sh, qe = X[1] >> sh, ip = X[2] >> sh, qp = X[3] >> sh, il = X[4] >> sh, ql = X[5] >> sh;

    const int64_t num = (ie - il) * ip + (qe - ql) * qp, den = ip * ip + qp * qp;
    int64_t ed = den ? (num * 65536) / den : 0;
    ed = ed > 65536 ? 65536 : ed < -65536 ? -65536 : ed;

    int64_t wn;
    if ((int64_t) st.epoch < (int64_t) cfg.pull_epochs) {
        if (st.have_prev) {
            int64_t cross = st.prev_ip * qp - st.prev_qp * ip;
            const int64_t dot = st.prev_ip * ip + st.prev_qp * qp;
            if (dot < 0) cross = -cross;
            const int64_t s = follow_abs(cross) + follow_abs(dot);
            const int64_t ef = s ? (cross * 65536) / s : 0;
            st.carr_int += (ef * cfg.kf) >> 16;
        }
        wn = st.carr_int;
    } else {
        const int64_t numc = ip >= 0 ? qp : -qp, denc = follow_abs(ip) + follow_abs(qp);
        const int64_t ec = denc ? (numc * 65536) / denc : 0;
        st.carr_int += (ec * cfg.ki) >> 16;
        wn = st.carr_int + ((ec * cfg.kp) >> 16);
    }

    st.carr_phase = (st.carr_phase + (uint64_t) N * (uint64_t) st.carr_step) & kCarrFracMask;
    const unsigned __int128 total = (unsigned __int128) st.code_frac + (unsigned __int128) N * (unsigned __int128) st.code_step;
    st.chip = (uint16_t) ((uint32_t) st.chip + (uint32_t) (uint64_t) (total >> GPSIQ_CODE_FRAC_BITS) - GPSIQ_CA_SEQ_LEN);
    st.code_frac = (uint64_t) total & kCodeFracMask;
    st.sample += N;
    st.prev_ip = ip; st.prev_qp = qp; st.have_prev = 1;
    st.epoch += 1;

    st.carr_step = wn;
    st.code_step = (uint64_t) ((int64_t) st.code_step0 + wn / 12320 + ((ed * cfg.kd) >> 16));
}

}  // namespace

template <int FMT>
__global__ __launch_bounds__(kFollowThreads) void follow_epochs(
    const uint8_t *__restrict__ src, uint64_t nsamp, const DeviceTables *__restrict__ tab, gpsiq_follow_cfg_t cfg,
    gpsiq_follow_state_t *__restrict__ states, gpsiq_follow_epoch_t *__restrict__ epochs, int max_epochs, int *__restrict__ counts,
    int per_launch)
{
    __shared__ uint32_t unit[512];
    __shared__ uint32_t ext[kPrnExtWords];
    __shared__ FollowEpoch ep;
    __shared__ int64_t part[kFollowWaves][kFollowSums];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, p = blockIdx.x;
    stage_unit<kFollowThreads>(tab, unit);
    if (tid < kPrnExtWords) ext[tid] = tab->prn_ext[states[p].prn - 1][tid];        // (the host has checked prn)

    gpsiq_follow_state_t st = {};
    int count = 0;
    if (tid == 0) { st = states[p]; count = counts[p]; }

    for (int e = 0; ; ++e) {
        if (tid == 0) {
            int go = 0;
            const int64_t cs = (int64_t) st.code_step;
            if (st.status == GPSIQ_FOLLOW_RUNNING && e < per_launch) {
                if (cs < kFollowCodeMin || cs >= kFollowCodeEnd || st.carr_step <= -kFollowCarrEnd || st.carr_step >= kFollowCarrEnd) {
                    st.status = GPSIQ_FOLLOW_RANGE;
                } else {
                    const uint32_t N = follow_len(st.chip, st.code_frac, st.code_step);
                    if (st.sample > nsamp || (uint64_t) N > nsamp - st.sample) {
                        st.status = GPSIQ_FOLLOW_SPAN_END;
                    } else if (count >= max_epochs) {
                        st.status = GPSIQ_FOLLOW_FULL;
                    } else {
                        go = 1;
                        ep.m = st.sample; ep.c = st.code_step; ep.w = (uint64_t) st.carr_step; ep.phase = st.carr_phase; ep.N = N;
                        // early: T0 + spacing (the chip may reach 1023: the lanes reduce it); late: T0 - spacing, one period on where
                        // that is negative
                        const uint64_t fe = st.code_frac + cfg.spacing;
                        ep.chip[0] = (uint32_t) st.chip + (uint32_t) (fe >> GPSIQ_CODE_FRAC_BITS); ep.frac[0] = fe & kCodeFracMask;
                        ep.chip[1] = st.chip; ep.frac[1] = st.code_frac;
                        if (st.code_frac >= cfg.spacing) {
                            ep.chip[2] = st.chip; ep.frac[2] = st.code_frac - cfg.spacing;
                        } else {
                            ep.chip[2] = st.chip ? (uint32_t) st.chip - 1u : GPSIQ_CA_SEQ_LEN - 1u;
                            ep.frac[2] = st.code_frac + (kCodeFracMask + 1u) - cfg.spacing;
                        }
                    }
                }
            }
            ep.go = go;
        }
        __syncthreads();                                        // (also behind the staging of unit and ext, the first time)
        if (!ep.go) break;                                      // every thread reads the same word: the whole workgroup leaves together

        const uint32_t N = ep.N;
        const uint64_t m = ep.m, c = ep.c, w = ep.w, phase = ep.phase;
        int64_t acc[kFollowSums] = {0, 0, 0, 0, 0, 0};
        for (uint32_t row = (uint32_t) wave; row * kFollowRow < N; row += kFollowWaves) {
            const uint32_t n = row * kFollowRow + (uint32_t) lane;
            int si, sq;
            load_iq<FMT>(src, m + (uint64_t) n, &si, &sq, n < N);           // past the epoch: nothing is read, (0, 0) adds nothing
            const uint64_t P = phase + w * (uint64_t) n;                    // mod 2^64, a multiple of 2^59
            const uint32_t v = unit[(uint32_t) ((P & kCarrFracMask) >> (GPSIQ_CARR_FRAC_BITS - 9))];
            const int rc = (int16_t) (v & 0xffffu), rs = (int32_t) v >> 16;
            const int yi = si * rc + sq * rs, yq = sq * rc - si * rs;       // each product below 2^24
            const unsigned __int128 adv = (unsigned __int128) c * (unsigned __int128) n;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const uint32_t k = (ep.chip[t] + (uint32_t) (uint64_t) ((adv + (unsigned __int128) ep.frac[t]) >> GPSIQ_CODE_FRAC_BITS)) % GPSIQ_CA_SEQ_LEN;
                const bool neg = (ext[k >> 5] >> (k & 31)) & 1u;
                acc[2 * t] += (int64_t) (neg ? -yi : yi);
                acc[2 * t + 1] += (int64_t) (neg ? -yq : yq);
            }
        }
#pragma unroll
        for (int i = 0; i < kFollowSums; ++i) {
            for (int off = 32; off >= 1; off >>= 1) acc[i] += __shfl_xor(acc[i], off, 64);
            if (lane == 0) part[wave][i] = acc[i];
        }
        __syncthreads();
        if (tid == 0) {
            int64_t X[kFollowSums];
            for (int i = 0; i < kFollowSums; ++i) {
                X[i] = 0;
                for (int v = 0; v < kFollowWaves; ++v) X[i] += part[v][i];
            }
            follow_close(st, cfg, N, X, epochs + (uint64_t) p * (uint64_t) max_epochs + (uint64_t) count);
            ++count;
        }
        // (ep is next written by the state thread, behind the barrier above: no wave reads it again before the barrier at the top;
        // part is next written behind that barrier, which the state thread reaches only after it has read part)
    }
    if (tid == 0) {
        for (int i = 0; i < 7; ++i) st.reserved[i] = 0;
        states[p] = st;
        counts[p] = count;
    }
}

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_follow.cpp looks up.
FollowFn follow_kernel(int fmt)
{
    return fmt == GPSIQ_SC16 ? follow_epochs<GPSIQ_SC16> : fmt == GPSIQ_SC08 ? follow_epochs<GPSIQ_SC08> : nullptr;
}
}  // namespace gpsiq
