// filter_plan.cpp -- csrc/gpsiq_filter_plan.h, the header gpsiq_filter / gpsiq_generate_batch_filtered plan with and build the matrix
// kernel's operand with, as a stand-alone program.  tests/test_filter_ref.py compiles and asks it, and also runs it built with -fsanitize=address,undefined.
// TEST INFRASTRUCTURE.  One request per line of stdin:
//   plan   NSAMP IN_SIZE NTAPS DECIM PHASE MAX_TAP FORCE   -> "nothing nout=0 next=.." |
//                                                            "kernel=.. nout=.. next=.. grid=.. threads=.. run=.. steps=.. runs=.. lds=.."
//   piece  NBLOCKS NSAMP SRC_BLOCK_BYTES OVERRIDE          -> "piece=.."
//   planes NTAPS DECIM SEED KIND                           -> "planes ok rows=.. steps=.."   (KIND 0: random taps, 1: taps at the sum bound
//                                                            and on the digit seams, stream at its extremes)
//   limits                                                 -> "min_taps=.. max_tap=.. max_run=.. threads=.."
// Every answer is first held to what a plan must hold whatever was asked: the runs cover the outputs exactly once, the window of a
// run fits the LDS it asks for and that fits a workgroup, the grid is non-empty and within its limit.  `planes` multiplies the host's
// two digit planes against a window of int8 samples in plain C++, in filter_mfma's own arithmetic -- int32 partial sums, then
// P0 + 256 P1 -- and compares every row of the tile with the direct real sum: the CPU proof of the operand layout and of the k range.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

static uint64_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t) (rng_state >> 33); }
static int rnd_in(int lo, int hi) { return lo + (int) (rnd() % (uint32_t) (hi - lo + 1)); }

// one tile column: 8 outputs from a window of 7 decim + ntaps int8 samples, first output at window sample ntaps - 1
static int planes(int ntaps, int decim, uint64_t seed, int kind)
{
    rng_state = seed * 2654435761ULL + 12345;
    std::vector<int16_t> taps((size_t) ntaps, 0);
    if (kind == 0) {
        const int lim = 65535 / ntaps > kFiltMfmaMaxTap ? kFiltMfmaMaxTap : 65535 / ntaps;      // (one or two taps: what the matrix path serves)
        for (auto &t : taps) t = (int16_t) rnd_in(-lim, lim);
    } else {                                                          // the sum bound exactly, entries on the digit seams first
        static const int seams[] = {32639, -32639, 127, -128, 128, -127, -129, 255, -256, 256};
        long left = 65535;
        for (size_t i = 0; i < taps.size() && left > 0; ++i) {
            int v = i < 10 ? seams[(i + seed) % 10] : rnd_in(-300, 300);
            if (i + 1 == taps.size() || std::labs((long) v) > left) v = (int) (left > 32639 ? 32639 : left) * ((rnd() & 1) ? 1 : -1);
            taps[i] = (int16_t) v;
            left -= std::labs((long) v);
        }
    }
    long mag = 0;
    int max_tap = -32768;
    for (const int16_t t : taps) { mag += std::labs((long) t); if (t > max_tap) max_tap = t; }
    if (mag > kFiltTapSum || !filter_mfma_serves(1, max_tap)) { std::fprintf(stderr, "the test's own taps are outside the matrix path\n"); return 2; }
    const int steps = filter_mfma_steps(ntaps, decim), kbytes = steps * kFiltK, wsamp = 7 * decim + ntaps;
    // the window: samples [0, wsamp), the first `zeros` of them the contract's zeros (before the head); past wsamp: padding, zeros
    const int zeros = (int) (seed % 3) * (ntaps / 3);
    std::vector<int32_t> x(2 * (size_t) (kbytes / 2 + 1), 0);
    for (int m = zeros; m < wsamp; ++m)
        for (int c = 0; c < 2; ++c) x[2 * (size_t) m + c] = kind == 1 ? ((rnd() & 1) ? -128 : 127) : (rnd() % 8 == 0 ? ((rnd() & 1) ? -128 : 127) : rnd_in(-128, 127));
    std::vector<int8_t> pl((size_t) filter_mfma_plane_bytes(steps));
    filter_build_planes(taps.data(), ntaps, decim, steps, pl.data());
    const size_t plane = (size_t) steps * kFiltK * 16;
    const auto a_at = [&](int p, int row, int k) { return (int) pl[p * plane + ((size_t) (k / kFiltK) * 64 + (size_t) (16 * ((k % kFiltK) / 16) + row)) * 16 + (size_t) (k % 16)]; };
    for (int row = 0; row < 16; ++row) {
        const int jj = row >> 1, c = row & 1;
        int64_t want = 0;                                             // the direct sum of the contract
        for (int k = 0; k < ntaps; ++k) want += (int64_t) taps[(size_t) k] * x[2 * (size_t) ((ntaps - 1) + jj * decim - k) + c];
        int32_t p0 = 0, p1 = 0;
        for (int k = 0; k < kbytes; ++k) { p0 += a_at(0, row, k) * x[(size_t) k]; p1 += a_at(1, row, k) * x[(size_t) k]; }
        if (std::labs((long) p0) > (1L << 23) || std::labs((long) p1) > (1L << 16)) { std::fprintf(stderr, "a partial sum leaves its bound\n"); return 1; }
        const int32_t got = p0 + 256 * p1;                            // filter_mfma's int32 recombination
        if (want >= (int64_t) 1 << 31 || want < -((int64_t) 1 << 31) || got != (int32_t) want) {
            std::fprintf(stderr, "row %d: planes give %d, the direct sum %lld\n", row, got, (long long) want);
            return 1;
        }
    }
    return std::printf("planes ok rows=16 steps=%d\n", steps) < 0;
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
        } else if (!std::strcmp(what, "planes")) {
            if (std::scanf("%lld %lld %lld %lld", &a, &b, &c, &d) != 4) return 2;
            if (a < 1 || a > kFiltMaxTaps || b < 1 || b > kFiltMaxDecim) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (int rc = planes((int) a, (int) b, (uint64_t) c, (int) d)) return rc;
        } else if (!std::strcmp(what, "limits")) {
            std::printf("min_taps=%d max_tap=%d max_run=%d threads=%d\n", kFiltMfmaMinTaps, kFiltMfmaMaxTap, kFiltMaxRun, kFiltThreads);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
