// acquire_plan.cpp -- plan_acquire() of csrc/gpsiq_acquire_plan.h, the header gpsiq_acquire itself plans with, as a stand-alone
// program: which kernels, grids and scratch a call takes.  tests/_acquire_plan.py compiles and asks it; tests/test_acquire_ref.py
// also runs it built with -fsanitize=address,undefined.  Host code only.  TEST INFRASTRUCTURE.
//   acquire_plan NSAMP SAMPLE_SIZE NPRN NDOPP NSHIFT NCOH NNONCOH HOP FORCE        one request (FORCE: - default, generic, mfma, nofast:
//                                                                                    the default of a library whose matrix path is behind the knob)
//   acquire_plan -                                                                  the same, one request per line of stdin
// answer: "nothing", or "kernel=mfma digits=3 span=.. cells=.. corr_cells=.. gx=.. gy=.. gz=.. row_tiles=.. npad=.. scratch=.. wipe_grid=..
//          mx=.. my=.. mz=.. ksteps=.. lds=.. peak_grid=.."
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gpsiq_acquire_plan.h"

static int answer(long long nsamp, int ss, int nprn, int ndopp, long long nshift, long long ncoh, long long nnoncoh, long long hop, const char *force)
{
    using namespace gpsiq;
    const bool nofast = !std::strcmp(force, "nofast");
    const AcquirePlan p = plan_acquire(nsamp, ss, nprn, ndopp, nshift, ncoh, nnoncoh, hop, !std::strcmp(force, "generic"),
                                       nofast ? false : !std::strcmp(force, "-") ? kAcqFastDefault : true, !std::strcmp(force, "mfma"));
    if (p.kind != kPlanLaunch) return std::printf("nothing\n") < 0;
    // what every plan must hold, whatever was asked
    bool ok = p.span <= (uint64_t) nsamp && p.cells == (uint64_t) nprn * ndopp * (uint64_t) nshift && (uint64_t) p.gx * kAcqThreads >= (uint64_t) nshift &&
              p.peak_grid * (kAcqThreads / 64) >= (uint64_t) nprn * ndopp && p.peak_grid < (UINT64_C(1) << 31);
    if (p.kernel == kAcquireMfma) {
        // every byte a k-step can touch lies inside its tile's planes; the code copies fit 64 KiB; the planes fit the cap; the grids fit a launch
        const uint64_t last = (uint64_t) (p.mx - 1) * kAcqBlockShifts + ((uint64_t) ((nnoncoh - 1) * hop) & ~UINT64_C(15)) + (uint64_t) p.ksteps * kAcqK;
        ok = ok && last <= p.npad && p.npad % 16 == 0 && p.span <= p.npad && p.scratch_bytes == (uint64_t) p.row_tiles * kAcqTileRows * p.npad &&
             p.scratch_bytes <= kAcqScratchCap && p.lds_bytes <= 65536u - 256u && p.lds_bytes == 16u * (unsigned) (ncoh + kAcqCopyPad) && p.row_tiles * kAcqBinsPerTile >= ndopp &&
             (uint64_t) p.mx * kAcqBlockShifts >= (uint64_t) nshift && p.my * kAcqWaves >= (unsigned) p.row_tiles && p.my < 65536u && p.mz == (unsigned) nprn &&
             p.wipe_grid * kAcqThreads >= (uint64_t) p.row_tiles * kAcqBinsPerTile * (p.npad / 4) && p.wipe_grid < (UINT64_C(1) << 31) &&
             p.ksteps == ncoh / kAcqK + 5 && p.digits == (ss == 1 ? 3 : 4);
    }
    if (!ok) {
        std::fprintf(stderr, "plan does not hold its own invariants\n");
        return 1;
    }
    return std::printf("kernel=%s digits=%d span=%" PRIu64 " cells=%" PRIu64 " corr_cells=%" PRIu64 " gx=%u gy=%u gz=%u row_tiles=%d npad=%" PRIu64
                       " scratch=%" PRIu64 " wipe_grid=%" PRIu64 " mx=%u my=%u mz=%u ksteps=%d lds=%u peak_grid=%" PRIu64 "\n",
                       acquire_kernel_name(p.kernel), p.digits, p.span, p.cells, p.corr_cells, p.gx, p.gy, p.gz, p.row_tiles, p.npad, p.scratch_bytes, p.wipe_grid,
                       p.mx, p.my, p.mz, p.ksteps, p.lds_bytes, p.peak_grid) < 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "-")) {
        long long nsamp, nshift, ncoh, nnoncoh, hop;
        int ss, nprn, ndopp;
        char force[16];
        while (std::scanf("%lld %d %d %d %lld %lld %lld %lld %15s", &nsamp, &ss, &nprn, &ndopp, &nshift, &ncoh, &nnoncoh, &hop, force) == 9)
            if (answer(nsamp, ss, nprn, ndopp, nshift, ncoh, nnoncoh, hop, force)) return 1;
        return 0;
    }
    if (argc != 10) {
        std::fprintf(stderr, "usage: %s NSAMP SAMPLE_SIZE NPRN NDOPP NSHIFT NCOH NNONCOH HOP -|generic|mfma|nofast   or   %s -\n", argv[0], argv[0]);
        return 2;
    }
    return answer(std::atoll(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoll(argv[5]), std::atoll(argv[6]),
                  std::atoll(argv[7]), std::atoll(argv[8]), argv[9]);
}
