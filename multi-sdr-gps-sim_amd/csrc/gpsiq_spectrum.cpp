// gpsiq_spectrum.cpp -- host side of gpsiq_spectrum (include/gpsiq_rows.h, "Spectrum"): checks, plan (gpsiq_spectrum_plan.h, pure and
// pinned on the CPU), the carrier table and the matrix kernel's table matrix with its cache, zeroing of the device result, kernel
// look-up (gpsiq_spectrum_kernels.hip holds the kernels and the table of those that exist), launch and copy-back.  libgpsiq_rows.so
// exports the typed call and reaches this through the plumbing entry "spectrum".
// Host code: nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_spectrum.h"
#include "gpsiq_spectrum_plan.h"
#include "gpsiq_tables.h"

using namespace gpsiq;

namespace {

static_assert(kSpecAuto == 0 && kSpecForceGeneric == 1 && kSpecForceMfma == 2, "forced_kernel's values (gpsiq_stage_call.h)");

// the coefficient of byte e = 2 n + c of a segment in X_comp[k]: Xi = I c + Q s, Xq = Q c - I s at idx = (k n T) mod 512
inline int twiddle(int k, int comp, int e, int T)
{
    const int idx = (k * (e >> 1) * T) & 511, cs = sin512(idx + 128), sn = sin512(idx);
    return comp == 0 ? ((e & 1) ? sn : cs) : ((e & 1) ? cs : -sn);
}

// The table matrix of (nfft, window) in two digit planes, fragment order (gpsiq_spectrum_geometry.h): lane l = (row i = l & 15, group
// g = l >> 4) of (row tile rt, k-step t) holds bytes j = 0..15, e = 64 t + 16 g + j, of A(i, e), row i = 2 kk + comp of bin 8 rt + kk.
void build_matrix(int nfft, int window, int8_t *pl)
{
    const int T = 512 / nfft, ksteps = spectrum_ksteps(nfft), row_tiles = spectrum_row_tiles(nfft);
    const size_t plane = (size_t) spectrum_plane_bytes(nfft);
    for (int rt = 0; rt < row_tiles; ++rt)
        for (int t = 0; t < ksteps; ++t)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 16; ++j) {
                    const int i = l & 15, g = l >> 4, k = kSpecTileBins * rt + (i >> 1), comp = i & 1, e = kSpecK * t + 16 * g + j;
                    int a = twiddle(k, comp, e, T);
                    if (window) a = 2 * a - twiddle((k + nfft - 1) & (nfft - 1), comp, e, T) - twiddle((k + 1) & (nfft - 1), comp, e, T);
                    const int d0 = ((a + 128) & 255) - 128, d1 = (a - d0) / 256;
                    const size_t at = (((size_t) rt * (size_t) ksteps + (size_t) t) * 64 + (size_t) l) * 16 + (size_t) j;
                    pl[at] = (int8_t) d0;
                    pl[plane + at] = (int8_t) d1;
                }
}

// the table (generic kernel) or the table matrix (matrix kernel) on the device, queued on s on first use.  The caller has made sure
// nothing queued earlier still reads the page-locked staging (every call ends synchronised); `have` is set by the caller once the
// call has ended well
int stage_table(SpectrumSet &k, hipStream_t s)
{
    if (k.have_table) return GPSIQ_OK;
    for (int i = 0; i < 512; ++i) k.h_table[i] = ((uint32_t) sin512(i + 128) & 0xffffu) | ((uint32_t) sin512(i) << 16);
    HIP_TRY(hipMemcpyAsync(k.d_table.get(), k.h_table.get(), 512 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    return GPSIQ_OK;
}

int stage_matrix(SpectrumSet &k, int nfft, int window, int slot, hipStream_t s)
{
    const size_t bytes = 2 * (size_t) spectrum_plane_bytes(nfft);
    HIP_TRY(k.d_mat[slot].reserve(bytes));
    if (k.have_mat[slot]) return GPSIQ_OK;
    HIP_TRY(k.h_mat.reserve(2 * (size_t) spectrum_plane_bytes(kSpecMaxFft)));
    build_matrix(nfft, window, reinterpret_cast<int8_t *>(k.h_mat.get()));
    HIP_TRY(hipMemcpyAsync(k.d_mat[slot].get(), k.h_mat.get(), bytes, hipMemcpyHostToDevice, s));
    return GPSIQ_OK;
}

}  // namespace

int gpsiq_spectrum_impl(gpsiq_ctx_t *c, int nsamp, int sample_size, const void *src, void *hip_stream, int nfft, int hop, int window, int navg, int shift,
                        uint64_t *power, int *ngroups, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    if (!spectrum_shape_ok(nfft, hop, window, navg))
        return fail(GPSIQ_E_ARG, "nfft %d in {64, 128, 256, 512}, hop %d nfft/2 or nfft, window %d 0 or 1, navg %d >= 1", nfft, hop, window, navg);
    if (shift < 0 || shift > kSpecMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kSpecMaxShift);
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (!src) return fail(GPSIQ_E_ARG, "null source");
    if ((uintptr_t) src & 3) return fail(GPSIQ_E_ARG, "source %p not 4-byte aligned", src);
    if (!power) return fail(GPSIQ_E_ARG, "null result");
    if (!spectrum_fits(sample_size, nfft, window, navg, shift))
        return fail(GPSIQ_E_RANGE, "navg %d at shift %d: the sum of a group could pass 2^64 - 1 (gpsiq_spectrum_min_shift gives %d)", navg, shift,
                    spectrum_min_shift(sample_size, nfft, window, navg));
    const SpectrumPlan p = plan_spectrum(nsamp, sample_size, nfft, hop, navg, forced_kernel("GPSIQ_SPECTRUM_KERNEL", "mfma"));
    if (ngroups) *ngroups = p.ngroups;
    if (kernel_ms) *kernel_ms = 0.0f;
    SpectrumSet &k = c->spec;
    k.last[0] = -1; k.last[1] = 0; k.last[2] = 0; k.last[3] = p.ngroups;
    if (!p.launch) return GPSIQ_OK;                                   // no whole group: nothing to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    const size_t cells = (size_t) p.ngroups * (size_t) nfft;
    if (int rc = k.reserve(cells)) return rc;
    const int slot = (nfft == 64 ? 0 : nfft == 128 ? 1 : nfft == 256 ? 2 : 3) * 2 + window;
    if (p.kernel == kSpecMfma) { if (int rc = stage_matrix(k, nfft, window, slot, s)) return rc; }
    else if (int rc = stage_table(k, s)) return rc;
    HIP_TRY(hipMemsetAsync(k.d_power.get(), 0, p.power_bytes, s));    // the workgroups add into it: zeroed per call
    HIP_TRY(hipEventRecord(k.t0.get(), s));
    const uint8_t *span = static_cast<const uint8_t *>(src);
    if (p.kernel == kSpecMfma) {
        const SpectrumMfmaFn kernel = spectrum_mfma_kernel(sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no matrix spectrum kernel for %d-byte samples", sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), p.lds, s, span, (const uint8_t *) k.d_mat[slot].get(), nfft, hop, shift, navg,
                           (uint32_t) ((uint64_t) p.ngroups * (uint64_t) navg), p.run, p.work, p.per, k.d_power.get());
    } else {
        const SpectrumGenericFn kernel = spectrum_generic_kernel(sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no spectrum kernel for %d-byte samples", sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, span, (const uint32_t *) k.d_table.get(), nfft, hop, window, shift, navg, p.per,
                           p.work, k.d_power.get());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(k.t1.get(), s));
    HIP_TRY(hipMemcpyAsync(k.h_power.get(), k.d_power.get(), p.power_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (p.kernel == kSpecMfma) k.have_mat[slot] = true; else k.have_table = true;
    std::memcpy(power, k.h_power.get(), p.power_bytes);
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, k.t0.get(), k.t1.get()));
    k.last[0] = p.kernel; k.last[1] = (long long) p.grid; k.last[2] = p.run;
    return GPSIQ_OK;
}

extern "C" int gpsiq_spectrum_last_plan(const gpsiq_ctx_t *c, long long out[4])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->spec.last[i];
    return GPSIQ_OK;
}
