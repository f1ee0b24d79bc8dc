// gpsiq_follow.cpp -- host side of gpsiq_follow (include/gpsiq_rows.h, "Follow"): checks, plan (gpsiq_follow_plan.h, pure and pinned on
// the CPU), kernel look-up (gpsiq_follow_kernels.hip holds the kernel and the table of its instantiations), the launches, copy-back.
// libgpsiq_rows.so exports the typed call and reaches this through the plumbing entry "follow".  Host code: nothing here decides device
// code, so the file is not one of the device sources behind gpsiq_kernels_id().
// The states live in device memory for the whole call.  A launch does a bounded number of epochs per satellite; after each the states
// and record counts come back (a few KiB) and the host launches again while any satellite is still running -- the very path a caller
// takes who continues from a returned state.
#include <cstdlib>
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_follow.h"
#include "gpsiq_follow_plan.h"

using namespace gpsiq;

static int check_follow(const gpsiq_ctx *c, int nsamp, int sample_size, const void *src, const gpsiq_follow_cfg_t *cfg, const gpsiq_follow_state_t *state,
                        int nprn, const void *epochs, int max_epochs, const int *nepochs)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (nprn < 1 || nprn > kFollowMaxPrn) return fail(GPSIQ_E_ARG, "%d satellites: 1 to %d", nprn, kFollowMaxPrn);
    if (max_epochs < 1) return fail(GPSIQ_E_ARG, "room for %d records per satellite: at least 1", max_epochs);
    if (!follow_args_ok(nsamp, sample_size, nprn, max_epochs))
        return fail(GPSIQ_E_ARG, "%d x %d records: more than %llu bytes", nprn, max_epochs, (unsigned long long) kFollowRecordCap);
    if (!cfg || !state || !epochs || !nepochs) return fail(GPSIQ_E_ARG, "null argument");
    const int64_t gain_end = INT64_C(1) << 46;
    if (cfg->spacing < 1 || cfg->spacing > (UINT64_C(1) << GPSIQ_CODE_FRAC_BITS)) return fail(GPSIQ_E_ARG, "tap spacing outside (0, 2^56]");
    if (cfg->pull_epochs < 0 || cfg->reserved) return fail(GPSIQ_E_ARG, "pull-in epochs %d / reserved %d", cfg->pull_epochs, cfg->reserved);
    for (int64_t k : {cfg->kf, cfg->kp, cfg->ki, cfg->kd})
        if (k < 0 || k >= gain_end) return fail(GPSIQ_E_ARG, "gain %lld outside [0, 2^46)", (long long) k);
    for (int p = 0; p < nprn; ++p) {
        const gpsiq_follow_state_t &s = state[p];
        if (s.prn < 1 || s.prn > 32) return fail(GPSIQ_E_ARG, "state %d: prn %d out of range 1..32", p, (int) s.prn);
        if (s.chip >= GPSIQ_CA_SEQ_LEN || s.code_frac >> GPSIQ_CODE_FRAC_BITS) return fail(GPSIQ_E_ARG, "state %d: code phase out of range", p);
        if (s.code_step0 < (UINT64_C(1) << 52) || s.code_step0 >> (GPSIQ_CODE_FRAC_BITS + 1)) return fail(GPSIQ_E_ARG, "state %d: nominal code step outside [2^52, 2^57)", p);
        if (s.carr_phase >> GPSIQ_CARR_FRAC_BITS) return fail(GPSIQ_E_ARG, "state %d: carrier phase out of range", p);
        const int64_t int_end = INT64_C(1) << GPSIQ_CARR_FRAC_BITS, prev_max = INT64_C(1) << 22;
        if (s.carr_int <= -int_end || s.carr_int >= int_end) return fail(GPSIQ_E_ARG, "state %d: frequency integrator out of range", p);
        if (s.prev_ip < -prev_max || s.prev_ip > prev_max || s.prev_qp < -prev_max || s.prev_qp > prev_max || s.have_prev > 1)
            return fail(GPSIQ_E_ARG, "state %d: previous prompt out of range", p);
    }
    if (!src) return fail(GPSIQ_E_ARG, "null source");
    if ((uintptr_t) src & 3) return fail(GPSIQ_E_ARG, "source %p not 4-byte aligned", src);
    return GPSIQ_OK;
}

int gpsiq_follow_impl(gpsiq_ctx_t *c, int nsamp, int sample_size, const void *src, void *hip_stream, const gpsiq_follow_cfg_t *cfg,
                      gpsiq_follow_state_t *state, int nprn, gpsiq_follow_epoch_t *epochs, int max_epochs, int *nepochs, float *kernel_ms)
{
    static_assert(sizeof(gpsiq_follow_epoch_t) == kFollowRecordBytes && sizeof(gpsiq_follow_state_t) == 88 && sizeof(gpsiq_follow_cfg_t) == 48, "layout");
    if (c) { c->fol.last[0] = -1; c->fol.last[1] = c->fol.last[2] = c->fol.last[3] = 0; }
    if (int rc = check_follow(c, nsamp, sample_size, src, cfg, state, nprn, epochs, max_epochs, nepochs)) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    const char *knob = std::getenv("GPSIQ_FOLLOW_EPOCHS_PER_LAUNCH");
    const FollowPlan p = plan_follow(nsamp, sample_size, nprn, max_epochs, knob ? std::atoll(knob) : 0);
    if (p.kind != kPlanLaunch) return fail(GPSIQ_E_ARG, "not a call");          // (the checks above and the planner's are the same list)
    const FollowFn kernel = follow_kernel(sample_size);
    if (!kernel) return fail(GPSIQ_E_DEVICE, "no follow kernel for %d-byte samples", sample_size);
    FollowSet &f = c->fol;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    if (int rc = f.reserve((size_t) p.records)) return rc;

    for (int i = 0; i < nprn; ++i) {
        f.h_state[i] = state[i];
        f.h_state[i].status = GPSIQ_FOLLOW_RUNNING;
        f.h_count[i] = 0;
    }
    HIP_TRY(hipMemcpyAsync(f.d_state.get(), f.h_state.get(), (size_t) nprn * sizeof(gpsiq_follow_state_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(f.d_count.get(), f.h_count.get(), (size_t) nprn * sizeof(int), hipMemcpyHostToDevice, s));
    float ms = 0.0f;
    int launches = 0;
    for (bool running = true; running; ) {
        if (launches >= p.max_launches) return fail(GPSIQ_E_DEVICE, "a satellite is still running after %d launches", launches);
        HIP_TRY(hipEventRecord(f.t0.get(), s));
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, static_cast<const uint8_t *>(src), (uint64_t) nsamp, c->d_tab.get(), *cfg,
                           f.d_state.get(), f.d_epochs.get(), max_epochs, f.d_count.get(), p.epochs_per_launch);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(f.t1.get(), s));
        HIP_TRY(hipMemcpyAsync(f.h_state.get(), f.d_state.get(), (size_t) nprn * sizeof(gpsiq_follow_state_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(f.h_count.get(), f.d_count.get(), (size_t) nprn * sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        float one = 0.0f;
        HIP_TRY(hipEventElapsedTime(&one, f.t0.get(), f.t1.get()));
        ms += one;
        ++launches;
        running = false;
        for (int i = 0; i < nprn; ++i) running = running || f.h_state[i].status == GPSIQ_FOLLOW_RUNNING;
    }
    for (int i = 0; i < nprn; ++i) {
        const int n = f.h_count[i];
        if (n < 0 || n > max_epochs) return fail(GPSIQ_E_DEVICE, "satellite %d came back with %d records of %d", i, n, max_epochs);
        if (n) HIP_TRY(hipMemcpyAsync(epochs + (size_t) i * (size_t) max_epochs, f.d_epochs.get() + (size_t) i * (size_t) max_epochs,
                                      (size_t) n * sizeof(gpsiq_follow_epoch_t), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < nprn; ++i) { state[i] = f.h_state[i]; nepochs[i] = f.h_count[i]; }
    if (kernel_ms) *kernel_ms = ms;
    f.last[0] = (long long) p.grid; f.last[1] = p.epochs_per_launch; f.last[2] = launches; f.last[3] = (long long) p.record_bytes;
    return GPSIQ_OK;
}

extern "C" int gpsiq_follow_last_plan(const gpsiq_ctx_t *c, long long out[4])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->fol.last[i];
    return GPSIQ_OK;
}
