// gpsiq_launch.cpp -- the launcher of the synthesis kernels: plan (gpsiq_launch_plan.h, pure and pinned on the CPU), look the
// kernel up (gpsiq_kernels.hip: the typed table of the instantiations that exist), launch.  Host code: nothing here decides
// device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include "gpsiq_ctx.h"

namespace gpsiq {

hipError_t launch_variant(int variant, const gpsiq_qchan_t *desc, int nchan, int nsamp, int sample_size,
                          void *dst, size_t block_stride, int block0, int nblocks,
                          const DeviceTables *tab, hipStream_t stream, const SynthClass &cls, void *scratch,
                          const noise::Launch &nz)
{
    static const SegPolicy policy = seg_policy_from_env();      // read once per process
    const SynthPlan p = plan_synth(variant, nsamp, nblocks, sample_size, cls, scratch != nullptr, {nz.tab != nullptr, nz.max_z, nz.mult != 0}, policy);
    if (p.kind == kPlanNothing) return hipSuccess;
    if (p.kind == kPlanNoPath) return hipErrorInvalidValue;      // the host refuses these first (check_launch)
    const dim3 grid(p.grid), block(p.threads);
    uint8_t *d = static_cast<uint8_t *>(dst);
    // every synthesis kernel starts with the same seven arguments; a plan without a kernel is an error, never another kernel
    auto launch = [&](auto kernel, auto... shape) {
        if (!kernel) return hipErrorInvalidDeviceFunction;
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, desc, nchan, nsamp, d, block_stride, block0, tab, shape...);
        return hipGetLastError();
    };
    const int fmt = sample_size;
    const bool half = p.H == 2;
    switch (p.variant) {
    case kGeneric: return launch(generic_kernel(fmt), p.tiles, p.tile_samples, nz.tab, nz.seed, nz.block, nz.mult, nz.qmax);
    case kRows:    return launch(rows_kernel(fmt), p.tiles);
    case kRowsX:   return launch(rowsx_kernel(fmt, p.slots), p.tiles);
    case kSegBoth: return launch(both_kernel(fmt, p.slots), p.tiles, p.wave_rows, p.big_wgs, p.big_blocks, p.tiles_small);
    case kSegMask: {
        uint64_t *masks = static_cast<uint64_t *>(scratch);
        hipLaunchKernelGGL(sign_masks_kernel(), dim3(p.pre_grid), dim3(kMaskThreads), 0, stream, desc, nchan, nsamp, block0, nblocks, tab, masks,
                           p.rows_total, p.rowgroups);
        return launch(mask_kernel(fmt, p.slots), masks, p.rows_total, p.tiles, p.wave_rows);
    }
    default: break;        // tile, seg, segh: one kernel family per stage that is on
    }
    if (p.family == kLevel)
        return launch(tile_level_kernel(fmt, p.slots, half, p.fast), p.tiles, p.wave_rows, p.big_wgs, p.big_blocks, p.tiles_small, nz.tab, nz.seed, nz.block,
                      nz.mult, nz.qmax);
    if (p.family == kNoise)
        return launch(tile_noise_kernel(fmt, p.slots, half, p.fast), p.tiles, p.wave_rows, p.big_wgs, p.big_blocks, p.tiles_small, nz.tab, nz.seed, nz.block);
    return launch(tile_kernel(fmt, p.slots, half, p.fast), p.tiles, p.wave_rows, p.big_wgs, p.big_blocks, p.tiles_small);
}

// GPSIQ_NCO_REFERENCE fix-up (apply_patches): four patches per wave, sixteen lanes each
hipError_t launch_patches(const gpsiq_qchan_t *desc, int nchan, int nsamp, int sample_size, void *dst, size_t block_stride,
                          int block0, int nblocks, const DeviceTables *tab, const gpsiq_patch_t *patches, int npatch,
                          hipStream_t stream, const noise::Launch &nz)
{
    if (npatch <= 0 || nblocks <= 0 || nsamp <= 0) return hipSuccess;
    const PatchFn k = patch_kernel(sample_size);
    if (!k) return hipErrorInvalidDeviceFunction;
    hipLaunchKernelGGL(k, dim3((unsigned) ((npatch + 3) / 4)), dim3(64), 0, stream, desc, nchan, nsamp, static_cast<uint8_t *>(dst), block_stride,
                       block0, nblocks, tab, patches, npatch, nz.tab, nz.seed, nz.block, nz.mult, nz.qmax);
    return hipGetLastError();
}

}  // namespace gpsiq
