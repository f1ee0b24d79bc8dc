// filter_plan.cpp -- csrc/gpsiq_filter_plan.h, the header gpsiq_filter / gpsiq_generate_batch_filtered plan with, as a stand-alone
// program.  tests/test_filter_ref.py compiles and asks it, and also runs it built with -fsanitize=address,undefined.
// TEST INFRASTRUCTURE.  One request per line of stdin:
//   plan   NSAMP IN_SIZE NTAPS DECIM PHASE MAX_TAP FORCE   -> "nothing nout=0 next=.." |
//                                                            "kernel=.. nout=.. next=.. grid=.. threads=.. run=.. steps=.. runs=.. lds=.."
//   piece  NBLOCKS NSAMP SRC_BLOCK_BYTES OVERRIDE          -> "piece=.."
//   limits                                                 -> "min_taps=.. max_tap=.. max_run=.. threads=.."
// Every answer is first held to what a plan must hold whatever was asked: the runs cover the outputs exactly once, the window of a
// run fits the LDS it asks for and that fits a workgroup, the grid is non-empty and within its limit.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "gpsiq_filter_plan.h"

using namespace gpsiq;

static int show(const FilterPlan &p, int ntaps, int decim)
{
    if (!p.launch) return std::printf("nothing nout=%d next=%d\n", p.nout, p.next_phase) < 0;
    const uint64_t window = ((uint64_t) p.run - 1) * (uint64_t) decim + (uint64_t) ntaps;      // samples of a full run's window
    bool ok = p.nout > 0 && p.run >= kFiltThreads && p.run <= kFiltMaxRun && p.run % kFiltThreads == 0 && p.threads == (unsigned) kFiltThreads &&
              p.runs * (uint64_t) p.run >= (uint64_t) p.nout && (p.runs - 1) * (uint64_t) p.run < (uint64_t) p.nout && p.grid >= 1 &&
              p.grid <= kFiltMaxGrid && (uint64_t) p.grid <= p.runs && (p.runs <= kFiltMaxGrid ? p.grid == p.runs : p.grid == kFiltMaxGrid) &&
              p.lds + 64 <= 65536;
    if (p.kernel == kFiltGeneric) ok = ok && p.steps == 0 && p.lds == 4 * window + 4 * (uint64_t) ntaps && window <= (uint64_t) kFiltGenericWindow;
    else
        ok = ok && p.kernel == kFiltMfma && p.run % kFiltTileOutputs == 0 && (uint64_t) p.steps * kFiltK >= (uint64_t) (14 * decim + 2 * ntaps) &&
             p.steps <= kFiltMaxSteps &&
             // the last column of the last tile reads its k range inside the staged window, and the staged window holds every sample a row needs
             p.lds == (size_t) filter_mfma_plane_bytes(p.steps) + (size_t) filter_mfma_window_bytes(p.run, decim, p.steps) &&
             (uint64_t) filter_mfma_window_bytes(p.run, decim, p.steps) >= 2 * window;
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("kernel=%d nout=%d next=%d grid=%u threads=%u run=%d steps=%d runs=%" PRIu64 " lds=%zu\n", p.kernel, p.nout, p.next_phase, p.grid,
                       p.threads, p.run, p.steps, p.runs, p.lds) < 0;
}

int main()
{
    char what[16];
    long long a, b, c, d, e, f, g;
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "plan")) {
            if (std::scanf("%lld %lld %lld %lld %lld %lld %lld", &a, &b, &c, &d, &e, &f, &g) != 7) return 2;
            if (a < 0 || c < 1 || c > kFiltMaxTaps || d < 1 || d > kFiltMaxDecim || e < 0 || e >= d) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (show(plan_filter((int) a, (int) b, (int) c, (int) d, (int) e, (int) f, (int) g), (int) c, (int) d)) return 1;
        } else if (!std::strcmp(what, "piece")) {
            if (std::scanf("%lld %lld %lld %lld", &a, &b, &c, &d) != 4) return 2;
            const int n = filter_piece_blocks((int) a, (int) b, (size_t) c, (long) d);
            if (a > 0 && (n < 1 || n > a || (b > 0 && n > 1 && (long long) n * b > INT32_MAX))) { std::fprintf(stderr, "piece outside its bounds\n"); return 1; }
            std::printf("piece=%d\n", n);
        } else if (!std::strcmp(what, "limits")) {
            std::printf("min_taps=%d max_tap=%d max_run=%d threads=%d\n", kFiltMfmaMinTaps, kFiltMfmaMaxTap, kFiltMaxRun, kFiltThreads);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
