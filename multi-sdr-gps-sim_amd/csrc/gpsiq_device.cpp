// gpsiq_device.cpp — device half of the C-ABI in include/gpsiq.h: context, resident
// descriptors, explicit launches, the noise and level settings, the plumbing table.  HIP runtime only.  (The drop-in calls:
// gpsiq_batch.cpp, gpsiq_multi.cpp.)  There is deliberately no CPU path here: without a GPU gpsiq_create() fails.
// (The functions of the C-ABI and of the plumbing have their C linkage from include/*.h and gpsiq_plumbing.h.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <cstring>
#include <new>
#include <vector>

#include "gpsiq_ctx.h"
#include "gpsiq_noise_knots.h"
#include "gpsiq_pieces.h"

using namespace gpsiq;

// GPSIQ_TRACE=1 in the environment prints the host-side phase times of the batch call to stderr
double gpsiq_wall_ms()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double) ts.tv_sec * 1e3 + (double) ts.tv_nsec * 1e-6;
}

// Wait until no launch reads the buffer any more (every stream that used it), then forget the uses.
int gpsiq_wait_idle(gpsiq_ctx::DescBuf &b)
{
    if (b.upload_pending) {              // also when nothing was ever launched on the set: its staging is about to be rewritten
        HIP_TRY(hipEventSynchronize(b.uploaded.get()));
        b.upload_pending = false;
    }
    if (!b.in_use) return GPSIQ_OK;
    for (auto &u : b.use)
        if (u.active) { HIP_TRY(hipEventSynchronize(u.ev.get())); u.active = false; }
    b.in_use = false;
    return GPSIQ_OK;
}

// Record that stream s has just launched work reading the buffer.
int gpsiq_mark_use(gpsiq_ctx::DescBuf &b, hipStream_t s)
{
    gpsiq_ctx::DescBuf::Use *slot = nullptr;
    for (auto &u : b.use)
        if (u.active && u.s == s) { slot = &u; break; }
    if (!slot)
        for (auto &u : b.use)
            if (!u.active) { slot = &u; break; }
    if (!slot) {
        // more streams than events: put this stream behind the first tracked one, whose event it then re-records
        slot = &b.use[0];
        HIP_TRY(hipStreamWaitEvent(s, slot->ev.get(), 0));
    }
    HIP_TRY(slot->ev.ensure());
    HIP_TRY(hipEventRecord(slot->ev.get(), s));
    slot->s = s; slot->active = true;
    b.in_use = true;
    return GPSIQ_OK;
}

// The scaled noise table (include/gpsiq.h, "Receiver noise"): S[k] = rint((sigma*c) * K[k] * 2^-12), the same for the tail, in
// double arithmetic that is exact here and in numpy (the library builds with -ffp-contract=off).
static long noise_table(double sigma, gpsiq::noise::Entry *tab)
{
    const double s = sigma * GPSIQ_NOISE_C;
    int32_t S[512];
    for (int k = 0; k < 512; ++k) S[k] = (int32_t) std::rint(s * (double) gpsiq_noise_K[k] * 0x1p-12);
    for (int k = 0; k < 511; ++k) tab[k] = {S[k], S[k + 1] - S[k]};
    for (int f = 0; f < 64; ++f) tab[511 + f] = {(int32_t) std::rint(s * (double) gpsiq_noise_T[f] * 0x1p-12), 0};
    for (int e = gpsiq::noise::kEntries; e < gpsiq::noise::kTabEntries; ++e) tab[e] = {0, 0};
    return tab[gpsiq::noise::kEntries - 1].base;
}

static int pick_variant(const gpsiq_ctx *c, int variant) { return variant == kAuto ? auto_variant(c->cls.max_code_step) : variant; }

static int check_launch(const gpsiq_ctx *c, int block0, int nblocks, int nsamp, int sample_size,
                        const void *dst, size_t stride, int variant)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    if (nsamp < 0 || nblocks < 0 || block0 < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (!c->d_desc || nblocks > c->nblocks || block0 > c->nblocks - nblocks)        // no int overflow in the sum
        return fail(GPSIQ_E_STATE, "blocks [%d,+%d) not resident (have %d)", block0, nblocks, c->nblocks);
    if (!dst && nblocks && nsamp) return fail(GPSIQ_E_ARG, "null destination");
    if ((uintptr_t) dst & 3) return fail(GPSIQ_E_ARG, "destination %p not 4-byte aligned", dst);
    if (stride < block_bytes(nsamp, sample_size) || (stride & 3))
        return fail(GPSIQ_E_ARG, "block stride %zu too small or not a multiple of 4", stride);
    if (variant < 0 || variant >= kNumVariants) return fail(GPSIQ_E_ARG, "unknown variant %d", variant);
    const bool stages_ok = variant == kAuto || has_noise_path(variant);      // kAuto picks among kernels that have one
    if (c->noise.sigma > 0.0 && !stages_ok)
        return fail(GPSIQ_E_STATE, "variant %d has no receiver-noise path: turn noise off (gpsiq_set_noise) or use 0/generic/tile/seg/segh", variant);
    if (c->level.mult && !stages_ok)
        return fail(GPSIQ_E_STATE, "variant %d has no output-level path: turn the level off (gpsiq_set_level) or use 0/generic/tile/seg/segh", variant);
    if (int rc = gpsiq_check_level(c, sample_size)) return rc;
    if (variant == kSegHalf && c->cls.max_code_step > kHalfRowsMaxCodeStep)
        return fail(GPSIQ_E_RANGE, "half-row kernel needs f_code/fs <= 1 chip per sample");
    if (variant >= kRows && variant != kSegHalf && c->cls.max_code_step > kRowsMaxCodeStep)
        return fail(GPSIQ_E_RANGE, "row kernel needs f_code/fs <= 31/63 chip per sample");
    return GPSIQ_OK;
}

int gpsiq_create(gpsiq_ctx_t **out, int device)
{
    if (!out) return fail(GPSIQ_E_ARG, "null context pointer");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(GPSIQ_E_DEVICE, "no HIP device (%s); libgpsiq has no CPU path", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(GPSIQ_E_ARG, "device %d outside 0..%d", device, ndev - 1);
    HIP_TRY(hipSetDevice(device));
    gpsiq_ctx *c = new (std::nothrow) gpsiq_ctx;
    if (!c) return fail(GPSIQ_E_NOMEM, "out of memory");
    c->device = device;
    DeviceTables *h = new (std::nothrow) DeviceTables;
    if (!h) { delete c; return fail(GPSIQ_E_NOMEM, "out of memory"); }
    build_device_tables(h);
    e = c->stream.ensure();
    if (e == hipSuccess) e = c->stream2.ensure();
    if (e == hipSuccess) e = c->up_stream.ensure();
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = c->copy_stream[i].ensure();
        if (e == hipSuccess) e = c->chunk_done[i].ensure();
    }
    if (e == hipSuccess) e = c->d_tab.reserve(1);
    if (e == hipSuccess) e = hipMemcpy(c->d_tab.get(), h, sizeof(DeviceTables), hipMemcpyHostToDevice);
    delete h;
    if (e != hipSuccess) {
        gpsiq_destroy(c);
        return fail(GPSIQ_E_DEVICE, "context setup: %s", hipGetErrorString(e));
    }
    *out = c;
    return GPSIQ_OK;
}

// (every member of the context owns what it holds, gpsiq_own.h: nothing is listed here -- also for a context that
// gpsiq_create gave up on half-way)
void gpsiq_destroy(gpsiq_ctx_t *c)
{
    if (!c) return;
    (void) hipSetDevice(c->device);
    (void) hipDeviceSynchronize();
    delete c;
}

void *gpsiq_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void) fail(GPSIQ_E_NOMEM, "hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

void gpsiq_host_free(void *p)
{
    if (p) (void) hipHostFree(p);
}

// patch list against the set it belongs to: slot counts the block's ACTIVE channels (device order), sorted by (block, sample)
static int check_patches(const gpsiq_ctx::DescBuf &b, int nblocks, const gpsiq_patch_t *patches, int n)
{
    for (int i = 0; i < n; ++i) {
        const gpsiq_patch_t &p = patches[i];
        if ((int64_t) p.block >= nblocks || p.slot >= b.active_per_block[p.block] || p.lut > 511 || p.neg > 1)
            return fail(GPSIQ_E_RANGE, "patch %d (block %u, slot %u, lut %u) outside the resident descriptors", i, p.block, p.slot, p.lut);
        if (i && (patches[i - 1].block > p.block || (patches[i - 1].block == p.block && patches[i - 1].sample > p.sample)))
            return fail(GPSIQ_E_ARG, "patches not sorted by (block, sample) at %d", i);
    }
    return GPSIQ_OK;
}

// gpsiq_set_descriptors (+ the set's patches in the same step).  no_wait: the uploads are queued on the context's upload
// stream and the call returns; launches on the set wait for them on the device (the pieces of a batch: the render thread
// queues piece after piece without a round trip to the device in between).
int gpsiq_stage_descriptors(gpsiq_ctx_t *c, const gpsiq_qchan_t *q, int nblocks, int nchan, const gpsiq_patch_t *patches, int npatch, bool no_wait)
{
    if (!c || !q) return fail(GPSIQ_E_ARG, "null argument");
    if (nblocks < 0 || nchan < 1 || nchan > GPSIQ_MAX_CHAN) return fail(GPSIQ_E_ARG, "bad nblocks %d / nchan %d", nblocks, nchan);
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t) nblocks * (size_t) nchan;
    const int next = (c->cur + 1) % gpsiq_ctx::kSets;
    gpsiq_ctx::DescBuf &nb = c->buf[next];              // a set not being read by the latest launches
    // the launch from kSets sets ago may still be reading this buffer (and its staging may still be
    // the source of an upload): wait for exactly that, not for the whole device
    { int wrc = gpsiq_wait_idle(nb); if (wrc) return wrc; }
    HIP_TRY(nb.h.reserve(n));
    // Device copy is compacted per block: active channels first, unused slots (zeroed)
    // after them.  The sum over channels is commutative modulo 2^16, so slot order is free.
    // Validation + compaction run on host threads straight into the page-locked staging buffer,
    // BEFORE anything resident is touched: a rejected set leaves the previous one in place.
    struct PJob { const gpsiq_qchan_t *q; gpsiq_qchan_t *out; uint8_t *active; int nchan; uint64_t mx; int max_active; long max_amp; int rc; size_t bad; };
    nb.active_per_block.resize((size_t) nblocks);
    PJob pj = {q, nb.h.get(), nb.active_per_block.data(), nchan, 0, 0, 0, GPSIQ_OK, 0};
    const bool trace = std::getenv("GPSIQ_TRACE") != nullptr;
    const double t0 = trace ? gpsiq_wall_ms() : 0.0;
    parallel_for(nblocks, 0, 128, [](void *p, int b0, int b1) {
        PJob &j = *static_cast<PJob *>(p);
        uint64_t mx = 0;
        int max_active = 0;
        long max_amp = 0;
        for (int b = b0; b < b1; ++b) {
            int na = 0;
            long amp = 0;
            for (int s = 0; s < j.nchan; ++s) {
                const size_t i = (size_t) b * j.nchan + s;
                const gpsiq_qchan_t &d = j.q[i];
                if (!d.prn) continue;
                if (d.prn > 32 || d.chip0 >= GPSIQ_CA_SEQ_LEN || d.icode >= 20 || (d.code_frac >> GPSIQ_CODE_FRAC_BITS) ||
                    (d.code_step >> (GPSIQ_CODE_FRAC_BITS + 1)) || !(d.gain > -kMaxGain && d.gain < kMaxGain)) {
                    if (__sync_bool_compare_and_swap(&j.rc, GPSIQ_OK, d.prn > 32 ? GPSIQ_E_ARG : GPSIQ_E_RANGE)) j.bad = i;
                    continue;
                }
                if (d.code_step > mx) mx = d.code_step;
                amp += (long) (250.0 * std::fabs(d.gain));           // |(int)(table*gain)| <= (int)(250*|gain|), gps.c:2781-2782
                j.out[(size_t) b * j.nchan + na++] = d;
            }
            for (int s = na; s < j.nchan; ++s) std::memset(&j.out[(size_t) b * j.nchan + s], 0, sizeof(gpsiq_qchan_t));
            j.active[b] = (uint8_t) na;
            if (na > max_active) max_active = na;
            if (amp > max_amp) max_amp = amp;
        }
        for (uint64_t cur = j.mx; mx > cur && !__sync_bool_compare_and_swap(&j.mx, cur, mx); cur = j.mx) {}
        for (int cur = j.max_active; max_active > cur && !__sync_bool_compare_and_swap(&j.max_active, cur, max_active); cur = j.max_active) {}
        for (long cur = j.max_amp; max_amp > cur && !__sync_bool_compare_and_swap(&j.max_amp, cur, max_amp); cur = j.max_amp) {}
    }, &pj);
    if (pj.rc != GPSIQ_OK) return fail(pj.rc, "descriptor %zu outside the NCO format (prn %u)", pj.bad, q[pj.bad].prn);
    HIP_TRY(nb.d.reserve(n ? n : 1));
    if (npatch > 0) {                                   // before anything resident is touched, like the descriptors
        const int prc = check_patches(nb, nblocks, patches, npatch);
        if (prc) return prc;
        HIP_TRY(nb.d_patch.reserve(gpsiq_patch_room((size_t) npatch)));
        HIP_TRY(nb.h_patch.reserve(gpsiq_patch_room((size_t) npatch)));
        std::memcpy(nb.h_patch.get(), patches, (size_t) npatch * sizeof(gpsiq_patch_t));
    }
    if (n) {
        const double t1 = trace ? gpsiq_wall_ms() : 0.0;
        // on the context's upload stream (non-blocking, nothing else ever queued on it): overlaps whatever the caller's
        // streams and the context's own kernels are doing
        hipError_t e = hipMemcpyAsync(nb.d.get(), nb.h.get(), n * sizeof(gpsiq_qchan_t), hipMemcpyHostToDevice, c->up_stream.get());
        if (e == hipSuccess && npatch > 0)
            e = hipMemcpyAsync(nb.d_patch.get(), nb.h_patch.get(), (size_t) npatch * sizeof(gpsiq_patch_t), hipMemcpyHostToDevice, c->up_stream.get());
        if (e == hipSuccess && no_wait) {
            e = nb.uploaded.ensure();
            if (e == hipSuccess) e = hipEventRecord(nb.uploaded.get(), c->up_stream.get());
            if (e == hipSuccess) nb.upload_pending = true;
        } else if (e == hipSuccess) {
            e = hipStreamSynchronize(c->up_stream.get());
        }
        if (e != hipSuccess) return fail(GPSIQ_E_DEVICE, "descriptor upload: %s", hipGetErrorString(e));
        if (trace)
            std::fprintf(stderr, "[gpsiq trace] descriptors %d blocks: validate+compact %.2f ms, upload %s %.2f ms\n",
                         nblocks, t1 - t0, no_wait ? "queued" : "done", gpsiq_wall_ms() - t1);
    }
    c->cur = next;
    c->d_desc = nb.d.get();
    c->nblocks = nblocks; c->nchan = nchan; c->cls = {pj.mx, pj.max_active, pj.max_amp};
    nb.npatch = n ? npatch : 0;
    return GPSIQ_OK;
}

int gpsiq_set_descriptors(gpsiq_ctx_t *c, const gpsiq_qchan_t *q, int nblocks, int nchan)
{
    return gpsiq_stage_descriptors(c, q, nblocks, nchan, nullptr, 0, false);
}

int gpsiq_set_patches(gpsiq_ctx_t *c, const gpsiq_patch_t *patches, int n)
{
    if (!c || (n > 0 && !patches) || n < 0) return fail(GPSIQ_E_ARG, "bad patch list");
    HIP_TRY(hipSetDevice(c->device));
    gpsiq_ctx::DescBuf &cb = c->buf[c->cur];
    { const int prc = check_patches(cb, c->nblocks, patches, n); if (prc) return prc; }
    cb.npatch = 0;
    if (n == 0) return GPSIQ_OK;                      // launches in flight took their count with them
    // launches of THIS set may still be applying the list that is replaced (the other buffer's launches have their own)
    { int wrc = gpsiq_wait_idle(cb); if (wrc) return wrc; }
    HIP_TRY(cb.d_patch.reserve(gpsiq_patch_room((size_t) n)));
    hipError_t e = hipMemcpyAsync(cb.d_patch.get(), patches, (size_t) n * sizeof(gpsiq_patch_t), hipMemcpyHostToDevice, c->up_stream.get());
    if (e == hipSuccess) e = hipStreamSynchronize(c->up_stream.get());
    if (e != hipSuccess) return fail(GPSIQ_E_DEVICE, "patch upload: %s", hipGetErrorString(e));
    cb.npatch = n;
    return GPSIQ_OK;
}

int gpsiq_set_nco_mode(gpsiq_ctx_t *c, int mode)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (mode != GPSIQ_NCO_FIXED && mode != GPSIQ_NCO_REFERENCE) return fail(GPSIQ_E_ARG, "unknown NCO mode %d", mode);
    if (mode != c->nco_mode) c->carry = {};
    c->nco_mode = mode;
    return GPSIQ_OK;
}

// kernel + patches of blocks [block0, block0+nblocks) on stream s; marks the descriptor buffer as in use
// (nbase: absolute block index of the resident set's block 0, for the receiver noise)
static int launch_on(gpsiq_ctx *c, int v, int block0, int nblocks, int nsamp, int sample_size, void *dst, size_t stride, hipStream_t s,
                     uint64_t nbase)
{
    const gpsiq::noise::Launch nz = gpsiq_noise_at(c, nbase);
    const size_t need = variant_scratch_bytes(v, nsamp, nblocks);
    // growing is rare (the first launch of a shape); the free inside reserve() waits for whatever still uses the old buffer
    HIP_TRY(c->d_scratch.reserve(need));
    if (c->buf[c->cur].upload_pending) HIP_TRY(hipStreamWaitEvent(s, c->buf[c->cur].uploaded.get(), 0));    // a set staged without waiting
    hipError_t e = launch_variant(v, c->d_desc, c->nchan, nsamp, sample_size, dst, stride, block0, nblocks, c->d_tab.get(), s,
                                  c->cls, need ? c->d_scratch.get() : nullptr, nz);
    if (e == hipSuccess && c->buf[c->cur].npatch)
        e = launch_patches(c->d_desc, c->nchan, nsamp, sample_size, dst, stride, block0, nblocks, c->d_tab.get(), c->buf[c->cur].d_patch.get(),
                           c->buf[c->cur].npatch, s, nz);
    if (e != hipSuccess) return fail(GPSIQ_E_DEVICE, "launch: %s", hipGetErrorString(e));
    if (nblocks > 0 && nsamp > 0) return gpsiq_mark_use(c->buf[c->cur], s);
    return GPSIQ_OK;
}

int gpsiq_launch_abs(gpsiq_ctx *c, int block0, int nblocks, int nsamp, int sample_size, void *dst, size_t block_stride_bytes,
                     hipStream_t s, int variant, uint64_t nbase)
{
    int rc = check_launch(c, block0, nblocks, nsamp, sample_size, dst, block_stride_bytes, variant);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return launch_on(c, pick_variant(c, variant), block0, nblocks, nsamp, sample_size, dst, block_stride_bytes, s, nbase);
}

// an explicit launch renders resident block b as absolute block next_block + b and leaves the counter alone (it can be repeated)
int gpsiq_launch(gpsiq_ctx_t *c, int block0, int nblocks, int nsamp, int sample_size,
                 void *dst, size_t block_stride_bytes, void *hip_stream, int variant)
{
    return gpsiq_launch_abs(c, block0, nblocks, nsamp, sample_size, dst, block_stride_bytes, (hipStream_t) hip_stream, variant,
                            c ? c->noise.next_block : 0);
}

int gpsiq_synchronize(gpsiq_ctx_t *c, void *hip_stream)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t) hip_stream));
    return GPSIQ_OK;
}

int gpsiq_time_launches(gpsiq_ctx_t *c, int block0, int nblocks, int nsamp, int sample_size,
                        void *dst, size_t block_stride_bytes, void *hip_stream, int variant,
                        int iters, float *ms_per_launch)
{
    if (!ms_per_launch || iters < 1) return fail(GPSIQ_E_ARG, "bad timing arguments");
    int rc = check_launch(c, block0, nblocks, nsamp, sample_size, dst, block_stride_bytes, variant);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    const int v = pick_variant(c, variant);
    Event e0, e1;
    float ms = 0.f;
    hipError_t e = e0.ensure(hipEventDefault);
    if (e == hipSuccess) e = e1.ensure(hipEventDefault);
    if (e == hipSuccess) e = hipEventRecord(e0.get(), s);
    for (int i = 0; i < iters && e == hipSuccess && rc == GPSIQ_OK; ++i)
        rc = launch_on(c, v, block0, nblocks, nsamp, sample_size, dst, block_stride_bytes, s, c->noise.next_block);
    if (e == hipSuccess && rc == GPSIQ_OK) e = hipEventRecord(e1.get(), s);
    if (e == hipSuccess && rc == GPSIQ_OK) e = hipEventSynchronize(e1.get());
    if (e == hipSuccess && rc == GPSIQ_OK) e = hipEventElapsedTime(&ms, e0.get(), e1.get());
    if (rc != GPSIQ_OK) return rc;
    if (e != hipSuccess) return fail(GPSIQ_E_DEVICE, "timing: %s", hipGetErrorString(e));
    *ms_per_launch = ms / (float) iters;
    return GPSIQ_OK;
}

int gpsiq_num_variants(void) { return kNumVariants; }

const char *gpsiq_variant_name(int v) { return variant_name(v); }

// ---- receiver noise --------------------------------------------------------------------------------------------------------
// (the device table is replaced only when the device is idle: launches still queued read the one they were given)
int gpsiq_apply_noise(gpsiq_ctx *c, uint64_t seed, double sigma)
{
    HIP_TRY(hipSetDevice(c->device));
    if (sigma > 0.0) {
        gpsiq::noise::Entry tab[gpsiq::noise::kTabEntries];
        const long max_z = noise_table(sigma, tab);
        HIP_TRY(c->d_noise_tab.reserve(gpsiq::noise::kTabEntries));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(c->d_noise_tab.get(), tab, sizeof tab, hipMemcpyHostToDevice));
        c->noise.max_z = max_z;
    } else {
        c->noise.max_z = 0;
    }
    c->noise.seed = seed;
    c->noise.sigma = sigma > 0.0 ? sigma : 0.0;
    return GPSIQ_OK;
}

static int check_sigma(double sigma)
{
    if (!(std::isfinite(sigma) && sigma >= 0.0 && sigma <= 65536.0))
        return fail(GPSIQ_E_ARG, "noise sigma %g outside [0, 65536]", sigma);
    return GPSIQ_OK;
}

int gpsiq_set_noise(gpsiq_ctx_t *c, const gpsiq_noise_t *nz)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (!nz) return gpsiq_apply_noise(c, 0, 0.0);
    int rc = check_sigma(nz->sigma);
    if (rc) return rc;
    rc = gpsiq_apply_noise(c, nz->seed, nz->sigma);
    if (rc == GPSIQ_OK) c->noise.next_block = nz->next_block;
    return rc;
}

// ---- output level (include/gpsiq_rows.h; libgpsiq_rows.so's gpsiq_set_level arrives here through the plumbing entry "set_level") ----
int gpsiq_apply_level(gpsiq_ctx *c, uint32_t mult, int32_t qmax)
{
    if (mult && !c->d_zero_tab.get()) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(c->d_zero_tab.reserve(gpsiq::noise::kTabEntries));
        HIP_TRY(hipMemset(c->d_zero_tab.get(), 0, sizeof(gpsiq::noise::Entry) * gpsiq::noise::kTabEntries));
        HIP_TRY(hipDeviceSynchronize());
    }
    c->level.mult = mult;
    c->level.qmax = mult ? qmax : 0;
    return GPSIQ_OK;
}

static int set_level(gpsiq_ctx_t *c, const gpsiq_level_t *lv)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (!lv) return gpsiq_apply_level(c, 0, 0);
    if (lv->mult < 1u || lv->mult >= (1u << 24)) return fail(GPSIQ_E_ARG, "output level: mult %u outside [1, 2^24)", lv->mult);
    if (lv->qmax < 1 || lv->qmax > 32767) return fail(GPSIQ_E_ARG, "output level: qmax %d outside [1, 32767]", (int) lv->qmax);
    return gpsiq_apply_level(c, lv->mult, lv->qmax);
}

int gpsiq_noise_state(const gpsiq_ctx_t *c, gpsiq_noise_t *out)
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    out->seed = c->noise.seed;
    out->sigma = c->noise.sigma;
    out->next_block = c->noise.next_block;
    return GPSIQ_OK;
}

int gpsiq_noise_host(uint64_t seed, double sigma, uint64_t block, int nsamp, int32_t *iq)
{
    if ((!iq && nsamp > 0) || nsamp < 0) return fail(GPSIQ_E_ARG, "bad noise buffer");
    int rc = check_sigma(sigma);
    if (rc) return rc;
    gpsiq::noise::Entry tab[gpsiq::noise::kTabEntries];
    noise_table(sigma, tab);
    for (uint32_t l = 0; l < 64u && l < (uint32_t) nsamp; ++l) {                // lane-major: one stream at a time
        uint64_t x = gpsiq::noise::lane_start(seed, block, l);
        for (uint32_t n = l; n < (uint32_t) nsamp; n += 64u) {
            const uint32_t w = gpsiq::noise::xsh_rr(x);
            x = x * gpsiq::noise::kMul + gpsiq::noise::kInc;
            iq[2 * (size_t) n] = gpsiq::noise::z(tab, w & 0xffffu);
            iq[2 * (size_t) n + 1] = gpsiq::noise::z(tab, w >> 16);
        }
    }
    return GPSIQ_OK;
}

gpsiq::noise::Launch gpsiq_noise_at(const gpsiq_ctx *c, uint64_t block)
{
    gpsiq::noise::Launch nz;
    if (c->noise.sigma > 0.0) {
        nz.tab = c->d_noise_tab.get();
        nz.seed = c->noise.seed;
        nz.block = block;
        nz.max_z = c->noise.max_z;
    }
    if (c->level.mult) {
        nz.mult = c->level.mult;
        nz.qmax = c->level.qmax;
        if (!nz.tab) { nz.tab = c->d_zero_tab.get(); nz.block = block; }     // noise off: the level kernels draw zeros
    }
    return nz;
}

// ---- the one exported entry to the plumbing (gpsiq_plumbing.h) --------------------------------------------------------------
extern "C" void *gpsiq_plumbing(const char *name)
{
    static const struct { const char *name; void *fn; } table[] = {
#define GPSIQ_P(f) {#f, reinterpret_cast<void *>(&f)}
        GPSIQ_P(gpsiq_reference_chain), GPSIQ_P(gpsiq_reference_seeded), GPSIQ_P(gpsiq_reference_stats), GPSIQ_P(gpsiq_chain_inputs),
        GPSIQ_P(gpsiq_chain_maps), GPSIQ_P(gpsiq_chain_link), GPSIQ_P(gpsiq_chain_summary), GPSIQ_P(gpsiq_chain_fold), GPSIQ_P(gpsiq_chain_stats),
        GPSIQ_P(gpsiq_chain_maps_device), GPSIQ_P(gpsiq_chain_range), GPSIQ_P(gpsiq_chain_range_fold), GPSIQ_P(gpsiq_time_launches), GPSIQ_P(gpsiq_num_variants), GPSIQ_P(gpsiq_variant_name),
        GPSIQ_P(gpsiq_device_eval_stats), GPSIQ_P(gpsiq_device_eval_host_ms),
        GPSIQ_P(gpsiq_prn_code), GPSIQ_P(gpsiq_carrier_table), GPSIQ_P(gpsiq_generate_seeded), GPSIQ_P(gpsiq_noise_state), GPSIQ_P(gpsiq_noise_host),
        GPSIQ_P(gpsiq_despread_last_plan), GPSIQ_P(gpsiq_pack_last_plan), GPSIQ_P(gpsiq_acquire_last_plan), GPSIQ_P(gpsiq_follow_last_plan),
        GPSIQ_P(gpsiq_filter_last_plan), GPSIQ_P(gpsiq_spectrum_last_plan), GPSIQ_P(gpsiq_mix_last_plan),
        GPSIQ_P(gpsiq_resample_last_plan), GPSIQ_P(gpsiq_agc_last_plan), GPSIQ_P(gpsiq_agc_last_ms), GPSIQ_P(gpsiq_cfilter_last_plan),
        GPSIQ_P(gpsiq_array_last_plan), GPSIQ_P(gpsiq_stap_last_plan), GPSIQ_P(gpsiq_stap_beams_last_plan),
#undef GPSIQ_P
        // the internals libgpsiq_rows.so runs on (gpsiq_rows_link.cpp): one pool, one quantiser, one error text per thread
        {"set_error", reinterpret_cast<void *>(&gpsiq::set_error)}, {"parallel_for", reinterpret_cast<void *>(&gpsiq::parallel_for)},
        {"quantize_one", reinterpret_cast<void *>(&gpsiq::quantize_one)}, {"chain_carrier", reinterpret_cast<void *>(&gpsiq::chain_carrier)},
        {"set_level", reinterpret_cast<void *>(&set_level)},      // gpsiq_set_level of libgpsiq_rows.so (include/gpsiq_rows.h)
        {"despread", reinterpret_cast<void *>(&gpsiq_despread_impl)},      // gpsiq_despread of libgpsiq_rows.so (ibid.; gpsiq_despread.cpp)
        {"pack", reinterpret_cast<void *>(&gpsiq_pack_impl)},              // gpsiq_pack, gpsiq_unpack and gpsiq_generate_batch_packed of
        {"unpack", reinterpret_cast<void *>(&gpsiq_unpack_impl)},          // libgpsiq_rows.so (ibid., "Packed streams"; gpsiq_pack.cpp)
        {"generate_batch_packed", reinterpret_cast<void *>(&gpsiq_generate_batch_packed_impl)},
        {"acquire", reinterpret_cast<void *>(&gpsiq_acquire_impl)},        // gpsiq_acquire of libgpsiq_rows.so (ibid., "Acquisition"; gpsiq_acquire.cpp)
        {"follow", reinterpret_cast<void *>(&gpsiq_follow_impl)},          // gpsiq_follow of libgpsiq_rows.so (ibid., "Follow"; gpsiq_follow.cpp)
        {"filter", reinterpret_cast<void *>(&gpsiq_filter_impl)},          // gpsiq_filter and gpsiq_generate_batch_filtered of libgpsiq_rows.so
        {"generate_batch_filtered", reinterpret_cast<void *>(&gpsiq_generate_batch_filtered_impl)},      // (ibid., "Filter"; gpsiq_filter.cpp)
        {"spectrum", reinterpret_cast<void *>(&gpsiq_spectrum_impl)},      // gpsiq_spectrum of libgpsiq_rows.so (ibid., "Spectrum"; gpsiq_spectrum.cpp)
        {"mix", reinterpret_cast<void *>(&gpsiq_mix_impl)},                // gpsiq_mix and gpsiq_generate_batch_mixed of libgpsiq_rows.so
        {"generate_batch_mixed", reinterpret_cast<void *>(&gpsiq_generate_batch_mixed_impl)},            // (ibid., "Mix"; gpsiq_mix.cpp)
        {"resample", reinterpret_cast<void *>(&gpsiq_resample_impl)},      // gpsiq_resample and gpsiq_generate_batch_resampled of libgpsiq_rows.so
        {"generate_batch_resampled", reinterpret_cast<void *>(&gpsiq_generate_batch_resampled_impl)},    // (ibid., "Resample"; gpsiq_resample.cpp)
        {"agc", reinterpret_cast<void *>(&gpsiq_agc_impl)},                // gpsiq_agc and gpsiq_generate_batch_agc of libgpsiq_rows.so
        {"generate_batch_agc", reinterpret_cast<void *>(&gpsiq_generate_batch_agc_impl)},                // (ibid., "AGC"; gpsiq_agc.cpp)
        {"cfilter", reinterpret_cast<void *>(&gpsiq_cfilter_impl)},        // gpsiq_cfilter of libgpsiq_rows.so (ibid., "Complex filter and notch"; gpsiq_cfilter.cpp)
        {"array_cov", reinterpret_cast<void *>(&gpsiq_array_cov_impl)},    // gpsiq_array_cov and gpsiq_array_combine of libgpsiq_rows.so
        {"array_combine", reinterpret_cast<void *>(&gpsiq_array_combine_impl)},                          // (ibid., "Array"; gpsiq_array.cpp)
        {"stap_cov", reinterpret_cast<void *>(&gpsiq_stap_cov_impl)},      // gpsiq_stap_cov and gpsiq_stap_combine of libgpsiq_rows.so
        {"stap_combine", reinterpret_cast<void *>(&gpsiq_stap_combine_impl)},                            // (ibid., "Space-time array"; gpsiq_stap.cpp)
        {"stap_beams", reinterpret_cast<void *>(&gpsiq_stap_beams_impl)},  // gpsiq_stap_beams of libgpsiq_rows.so (ibid.; gpsiq_stap_beams.cpp)
    };
    if (!name) return nullptr;
    for (const auto &e : table)
        if (!std::strcmp(e.name, name)) return e.fn;
    return nullptr;
}
