// spectrum_plan.cpp -- csrc/gpsiq_spectrum_plan.h, the header gpsiq_spectrum plans with, as a stand-alone program.
// tests/test_spectrum_ref.py compiles and asks it, and also runs it built with -fsanitize=address,undefined.
// TEST INFRASTRUCTURE.  One request per line of stdin:
//   plan     NSAMP SAMPLE_SIZE NFFT HOP NAVG FORCE   -> "nothing nseg=.. ngroups=.." |
//                                                      "kernel=.. nseg=.. ngroups=.. grid=.. threads=.. run=.. per=.. work=.. lds=.. power_bytes=.."
//   fits     SAMPLE_SIZE NFFT WINDOW NAVG SHIFT      -> "fits=0|1"
//   minshift SAMPLE_SIZE NFFT WINDOW NAVG            -> "shift=.."   (-1: none up to the largest)
//   limits                                           -> "default_mfma=.. run=.. max_grid=.. mfma_grid=.. max_shift=.."
// Every plan is first held to what a plan must hold whatever was asked: the units or passes cover the segments that are read exactly
// once, the grid is non-empty and within its limit, the window of a pass fits the LDS it asks for and that fits a workgroup.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "gpsiq_spectrum_plan.h"

using namespace gpsiq;

static int show(const SpectrumPlan &p, int nfft, int hop, int navg)
{
    if (!p.launch) return std::printf("nothing nseg=%d ngroups=%d\n", p.nseg, p.ngroups) < 0;
    const uint64_t used = (uint64_t) p.ngroups * (uint64_t) navg;
    bool ok = p.ngroups > 0 && used <= (uint64_t) p.nseg && used + (uint64_t) navg > (uint64_t) p.nseg && p.grid >= 1 && p.work >= 1 &&
              p.power_bytes == (size_t) p.ngroups * (size_t) nfft * 8;
    if (p.kernel == kSpecGeneric)
        ok = ok && p.threads == (unsigned) (nfft < 256 ? nfft : 256) && p.run == kSpecRun && p.per * (uint64_t) p.run >= (uint64_t) navg &&
             (p.per - 1) * (uint64_t) p.run < (uint64_t) navg && p.work == (uint64_t) p.ngroups * p.per && p.grid <= kSpecMaxGrid &&
             (p.work <= kSpecMaxGrid ? p.grid == p.work : p.grid == kSpecMaxGrid) && p.lds == 0;
    else
        ok = ok && p.kernel == kSpecMfma && p.threads == (unsigned) kSpecThreads && p.run % kSpecTileCols == 0 && p.run >= kSpecTileCols &&
             p.run <= kSpecMaxColTiles * kSpecTileCols && p.work * (uint64_t) p.run >= used && (p.work - 1) * (uint64_t) p.run < used &&
             (uint64_t) p.grid * p.per >= p.work && ((uint64_t) p.grid - 1) * p.per < p.work && p.grid <= kSpecMfmaGrid &&
             p.lds == (size_t) spectrum_mfma_sums_bytes(nfft) + (size_t) spectrum_window_bytes(nfft, hop, p.run) && p.lds + 64 <= 65536 &&
             // the last column's last k-step ends inside the staged chunks, and every column start is 16-byte aligned
             (p.run - 1 + nfft / hop) * spectrum_chunk_stride(hop) == spectrum_window_bytes(nfft, hop, p.run) && spectrum_chunk_stride(hop) % 16 == 0 &&
             spectrum_mfma_sums_bytes(nfft) % 16 == 0;
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("kernel=%d nseg=%d ngroups=%d grid=%u threads=%u run=%d per=%" PRIu64 " work=%" PRIu64 " lds=%zu power_bytes=%zu\n", p.kernel, p.nseg,
                       p.ngroups, p.grid, p.threads, p.run, p.per, p.work, p.lds, p.power_bytes) < 0;
}

int main()
{
    char what[16];
    long long a, b, c, d, e, f;
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "plan")) {
            if (std::scanf("%lld %lld %lld %lld %lld %lld", &a, &b, &c, &d, &e, &f) != 6) return 2;
            if (a < 0 || a > INT32_MAX || e > INT32_MAX || !spectrum_shape_ok((int) c, (int) d, 0, (int) e) || (b != 1 && b != 2)) {
                std::fprintf(stderr, "request outside the ranges\n");
                return 2;
            }
            if (show(plan_spectrum((int) a, (int) b, (int) c, (int) d, (int) e, (int) f), (int) c, (int) d, (int) e)) return 1;
        } else if (!std::strcmp(what, "fits")) {
            if (std::scanf("%lld %lld %lld %lld %lld", &a, &b, &c, &d, &e) != 5) return 2;
            std::printf("fits=%d\n", spectrum_fits((int) a, (int) b, (int) c, (int) d, (int) e) ? 1 : 0);
        } else if (!std::strcmp(what, "minshift")) {
            if (std::scanf("%lld %lld %lld %lld", &a, &b, &c, &d) != 4) return 2;
            std::printf("shift=%d\n", spectrum_min_shift((int) a, (int) b, (int) c, (int) d));
        } else if (!std::strcmp(what, "limits")) {
            std::printf("default_mfma=%d run=%d max_grid=%u mfma_grid=%u max_shift=%d\n", kSpecMfmaDefault ? 1 : 0, kSpecRun, kSpecMaxGrid, kSpecMfmaGrid,
                        kSpecMaxShift);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
