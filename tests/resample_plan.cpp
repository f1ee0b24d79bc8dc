// resample_plan.cpp -- csrc/gpsiq_resample_plan.h, the header gpsiq_resample / gpsiq_generate_batch_resampled plan with, as a
// stand-alone program.  tests/test_resample_ref.py compiles and asks it, and also runs it built with -fsanitize=address,undefined.
// TEST INFRASTRUCTURE.  One request per line of stdin:
//   plan   NSAMP LOG2_PHASES NTAPS STEP POS0 FORCE   -> "nothing nout=0 next=.." |
//                                                      "kernel=.. nout=.. next=.. grid=.. threads=.. run=.. pad=.. runs=.. lds=.."
//   span   NSAMP POS0 STEP                           -> "nout=.. next=.."
//   piece  NBLOCKS NSAMP SRC_BLOCK_BYTES OVERRIDE    -> "piece=.."
//   most   SAMPLES STEP                              -> "most=.."      (the outputs a piece can give at the most)
//   limits                                           -> "default=.. run=.. unit=.. threads=.. max_grid=.. pad_step=.."
// Every plan is first held to what a plan must hold whatever was asked: the units cover the outputs exactly once, the table and the
// window of a run fit the LDS it asks for and that fits a workgroup, the grid is non-empty and within its limit.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "gpsiq_resample_plan.h"

using namespace gpsiq;

static int show(const ResamplePlan &p, int log2_phases, int ntaps, uint64_t step)
{
    if (!p.launch) return std::printf("nothing nout=%" PRIu64 " next=%" PRIu64 "\n", p.nout, p.next_pos) < 0;
    const size_t table = 4 * (size_t) resample_table_dwords(log2_phases, ntaps);
    bool ok = p.nout > 0 && p.threads == (unsigned) kRsThreads && p.run >= 1 && p.runs * (uint64_t) p.run >= p.nout &&
              (p.runs - 1) * (uint64_t) p.run < p.nout && p.grid >= 1 && p.grid <= kRsMaxGrid && (uint64_t) p.grid <= p.runs &&
              (p.runs <= kRsMaxGrid ? p.grid == p.runs : p.grid == kRsMaxGrid) && p.lds + 64 <= 65536 &&
              resample_tap_stride(ntaps) % 2 == 1 && 2 * resample_tap_stride(ntaps) >= ntaps;
    if (p.kernel == kRsGeneric) ok = ok && p.run == kRsGenericUnit && !p.pad && p.lds == table;
    else {
        // the largest window a run can need: its first output at the top of a sample, (run - 1) steps on
        const uint64_t window = (((uint64_t) (p.run - 1) * step + (kRsOne - 1)) >> 32) + (uint64_t) ntaps;
        const uint64_t room = (p.lds - table) / 4;
        ok = ok && p.kernel == kRsRows && p.run == kRsRun && p.run % kRsThreads == 0 && p.pad == (step >= kRsPadStep) && p.lds >= table &&
             (p.pad ? room >= window + ((window - 1) >> 5) : room >= window);
    }
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("kernel=%d nout=%" PRIu64 " next=%" PRIu64 " grid=%u threads=%u run=%d pad=%d runs=%" PRIu64 " lds=%zu\n", p.kernel, p.nout, p.next_pos,
                       p.grid, p.threads, p.run, (int) p.pad, p.runs, p.lds) < 0;
}

int main()
{
    char what[16];
    unsigned long long a, b, c, d, e, f;
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "plan")) {
            if (std::scanf("%llu %llu %llu %llu %llu %llu", &a, &b, &c, &d, &e, &f) != 6) return 2;
            if (a >= kRsMaxSpan || b > (unsigned) kRsMaxLog2Phases || c < 1 || c > (unsigned) kRsMaxTaps || ((1ull << b) + 1) * c > (unsigned) kRsMaxTable ||
                d < kRsMinStep || d > kRsMaxStep || e >= kRsMaxPos) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (show(plan_resample(a, (int) b, (int) c, d, e, (int) f), (int) b, (int) c, d)) return 1;
        } else if (!std::strcmp(what, "span")) {
            if (std::scanf("%llu %llu %llu", &a, &b, &c) != 3) return 2;
            if (a >= kRsMaxSpan || b >= kRsMaxPos || c < kRsMinStep || c > kRsMaxStep) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            uint64_t n = 0, next = 0;
            resample_span(a, b, c, &n, &next);
            std::printf("nout=%" PRIu64 " next=%" PRIu64 "\n", n, next);
        } else if (!std::strcmp(what, "piece")) {
            if (std::scanf("%llu %llu %llu %llu", &a, &b, &c, &d) != 4) return 2;
            const int n = resample_piece_blocks((int) a, (int) b, (size_t) c, (long) d);
            if (a > 0 && (n < 1 || (unsigned long long) n > a || (b > 0 && n > 1 && (unsigned long long) n * b > INT32_MAX))) { std::fprintf(stderr, "piece outside its bounds\n"); return 1; }
            std::printf("piece=%d\n", n);
        } else if (!std::strcmp(what, "most")) {
            if (std::scanf("%llu %llu", &a, &b) != 2) return 2;
            std::printf("most=%" PRIu64 "\n", resample_piece_outputs(a, b));
        } else if (!std::strcmp(what, "limits")) {
            std::printf("default=%d run=%d unit=%d threads=%d max_grid=%u pad_step=%" PRIu64 "\n", kRsDefaultKernel, kRsRun, kRsGenericUnit, kRsThreads, kRsMaxGrid,
                        kRsPadStep);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
