// mix_plan.cpp -- csrc/gpsiq_mix_plan.h, the header gpsiq_mix / gpsiq_generate_batch_mixed plan with, as a stand-alone program.
// tests/test_mix_ref.py compiles and asks it, and also runs it built with -fsanitize=address,undefined.
// TEST INFRASTRUCTURE.  One request per line of stdin:
//   plan   NSAMP M0 OUT_SIZE DST_ADDR FORCE            -> "nothing" | "kernel=.. grid=.. threads=.. lead=.. units=.."
//   piece  NBLOCKS NSAMP BLOCK_BYTES OVERRIDE          -> "piece=.."
//   limits                                             -> "rows_default=.. threads=.. max_grid=.. slot_bytes=.. max_terms=.. max_shift=.."
// Every answer is first held to what a plan must hold whatever was asked: the units cover the samples exactly once, every slot but
// the first and the last is whole, the first slot starts on a 16-byte boundary, the grid is non-empty and within its limit.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "gpsiq_mix_plan.h"

using namespace gpsiq;

static int show(const MixPlan &p, int nsamp, int out_size, uint64_t dst_addr)
{
    if (!p.launch) return std::printf("nothing\n") < 0;
    const uint64_t wgs = (p.units + kMixThreads - 1) / kMixThreads;
    bool ok = nsamp > 0 && p.threads == (unsigned) kMixThreads && p.grid >= 1 && p.grid <= kMixMaxGrid && (uint64_t) p.grid <= wgs &&
              (wgs <= kMixMaxGrid ? p.grid == wgs : p.grid == kMixMaxGrid);
    if (p.kernel == kMixGeneric) ok = ok && p.lead == 0 && p.units == (uint64_t) nsamp;
    else {
        const uint64_t per = (uint64_t) mix_slot_samples(out_size);
        ok = ok && p.kernel == kMixRows && p.lead >= 0 && (uint64_t) p.lead < per &&
             (dst_addr - (uint64_t) p.lead * 2 * (uint64_t) out_size) % kMixSlotBytes == 0 &&            // the first slot is aligned
             p.units * per >= (uint64_t) nsamp + (uint64_t) p.lead && (p.units - 1) * per < (uint64_t) nsamp + (uint64_t) p.lead;
    }
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("kernel=%d grid=%u threads=%u lead=%d units=%" PRIu64 "\n", p.kernel, p.grid, p.threads, p.lead, p.units) < 0;
}

int main()
{
    char what[16];
    long long a, c, e;
    unsigned long long b, d;
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "plan")) {
            if (std::scanf("%lld %llu %lld %llu %lld", &a, &b, &c, &d, &e) != 5) return 2;
            if (a < 0 || a > INT32_MAX || (c != 1 && c != 2) || (d & 3)) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (show(plan_mix((int) a, (uint64_t) b, (int) c, (uint64_t) d, (int) e), (int) a, (int) c, (uint64_t) d)) return 1;
        } else if (!std::strcmp(what, "piece")) {
            long long n, s, by, ov;
            if (std::scanf("%lld %lld %lld %lld", &n, &s, &by, &ov) != 4) return 2;
            const int got = mix_piece_blocks((int) n, (int) s, (size_t) by, (long) ov);
            if (n > 0 && (got < 1 || got > n || (s > 0 && got > 1 && (long long) got * s > INT32_MAX))) { std::fprintf(stderr, "piece outside its bounds\n"); return 1; }
            std::printf("piece=%d\n", got);
        } else if (!std::strcmp(what, "limits")) {
            std::printf("rows_default=%d threads=%d max_grid=%u slot_bytes=%d max_terms=%d max_shift=%d\n", kMixRowsDefault ? 1 : 0, kMixThreads, kMixMaxGrid,
                        kMixSlotBytes, kMixMaxTerms, kMixMaxShift);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
