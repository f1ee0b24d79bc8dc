// agc_plan.cpp -- csrc/gpsiq_agc_plan.h, the header gpsiq_agc / gpsiq_generate_batch_agc plan with, and the gain rule of
// csrc/gpsiq_agc_geometry.h, as a stand-alone program.  tests/test_agc_plan.py compiles and asks it, and also runs it built with
// -fsanitize=address,undefined.  TEST INFRASTRUCTURE.  One request per line of stdin:
//   plan   NSAMP WINDOW FILL MASK                    -> "nothing" |
//                                                      "nwin=.. next=.. measure=.. gains=.. apply=.. threads=.. units=.. cnt=.. zero=.. mult=.. mask=.. scratch=.."
//   span   NSAMP WINDOW FILL                         -> "nwin=.. next=.."
//   gain   SUMSQ COUNT TARGET MULT0 MIN MAX          -> "gain=.."
//   piece  NBLOCKS NSAMP SRC_BLOCK_BYTES OVERRIDE    -> "piece=.."
//   limits                                           -> "threads=.. unit=.. tile=.. apply_tile=.. tile_windows=.. lead_units=.."
// Every plan is first held to what a plan must hold whatever was asked: the tiles of either kernel cover the span exactly once, one
// thread per window, the regions of the scratch are aligned, in order and do not overlap, a tile touches no more windows than a
// workgroup has slots for.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "gpsiq_agc_plan.h"

using namespace gpsiq;

static int show(const AgcPlan &p, uint64_t nsamp, uint64_t window, uint64_t fill, bool mask)
{
    if (!p.launch) return std::printf("nothing\n") < 0;
    const uint64_t nwin = (fill + nsamp + window - 1) / window;
    bool ok = p.threads == (unsigned) kAgcThreads && p.nwin == nwin && p.next_fill == (fill + nsamp) % window && p.mask == mask &&
              (uint64_t) p.units * kAgcUnit >= nsamp && ((uint64_t) p.units - 1) * kAgcUnit < nsamp &&
              (uint64_t) p.measure_grid * kAgcTile >= nsamp && ((uint64_t) p.measure_grid - 1) * kAgcTile < nsamp &&
              (uint64_t) p.apply_grid * kAgcApplyTile >= nsamp && ((uint64_t) p.apply_grid - 1) * kAgcApplyTile < nsamp &&
              (uint64_t) p.gains_grid * kAgcThreads >= nwin && ((uint64_t) p.gains_grid - 1) * kAgcThreads < nwin &&
              p.off_cnt % 16 == 0 && p.off_mult % 16 == 0 && p.off_mask % 16 == 0 && p.off_cnt >= 8 * nwin && p.zero_bytes == p.off_cnt + 4 * nwin &&
              p.off_mult >= p.zero_bytes && p.off_mask >= p.off_mult + 4 * nwin && p.scratch_bytes == p.off_mask + (mask ? p.units : 0);
    // the windows a tile can touch at this window length, from any fill
    ok = ok && (kAgcTile + window - 2) / window + 1 <= (uint64_t) kAgcTileWindows + 1 && kAgcLeadUnits * kAgcUnit >= kAgcMaxHold;
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("nwin=%" PRIu64 " next=%u measure=%u gains=%u apply=%u threads=%u units=%u cnt=%zu zero=%zu mult=%zu mask=%zu scratch=%zu\n", p.nwin,
                       p.next_fill, p.measure_grid, p.gains_grid, p.apply_grid, p.threads, p.units, p.off_cnt, p.zero_bytes, p.off_mult, p.off_mask,
                       p.scratch_bytes) < 0;
}

int main()
{
    char what[16];
    unsigned long long a, b, c, d, e, f;
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "plan")) {
            if (std::scanf("%llu %llu %llu %llu", &a, &b, &c, &d) != 4) return 2;
            if (a > INT32_MAX || b > INT32_MAX || c > UINT32_MAX) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (show(plan_agc((int) a, (int) b, (uint32_t) c, d != 0), a, b, c, d != 0)) return 1;
        } else if (!std::strcmp(what, "span")) {
            if (std::scanf("%llu %llu %llu", &a, &b, &c) != 3) return 2;
            if (b < (unsigned) kAgcMinWindow || b > (unsigned) kAgcMaxWindow || c >= b) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            uint64_t n = 0;
            uint32_t next = 0;
            agc_span(a, (uint32_t) b, (uint32_t) c, &n, &next);
            std::printf("nwin=%" PRIu64 " next=%u\n", n, next);
        } else if (!std::strcmp(what, "gain")) {
            if (std::scanf("%llu %llu %llu %llu %llu %llu", &a, &b, &c, &d, &e, &f) != 6) return 2;
            if (a > kAgcMaxSum || b > kAgcMaxCount || c > kAgcMaxTarget || f > kAgcMaxMult) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            std::printf("gain=%u\n", agc_gain(a, b, (uint32_t) c, (uint32_t) d, (uint32_t) e, (uint32_t) f));
        } else if (!std::strcmp(what, "piece")) {
            if (std::scanf("%llu %llu %llu %llu", &a, &b, &c, &d) != 4) return 2;
            const int n = agc_piece_blocks((int) a, (int) b, (size_t) c, (long) d);
            if (a > 0 && (n < 1 || (unsigned long long) n > a || (b > 0 && n > 1 && (unsigned long long) n * b > INT32_MAX))) { std::fprintf(stderr, "piece outside its bounds\n"); return 1; }
            std::printf("piece=%d\n", n);
        } else if (!std::strcmp(what, "limits")) {
            std::printf("threads=%d unit=%d tile=%d apply_tile=%d tile_windows=%d lead_units=%d\n", kAgcThreads, kAgcUnit, kAgcTile, kAgcApplyTile, kAgcTileWindows,
                        kAgcLeadUnits);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
