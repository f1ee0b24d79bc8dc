// cfilter_plan.cpp -- csrc/gpsiq_cfilter_plan.h, the header gpsiq_cfilter plans with and builds its matrix operand with, as a
// stand-alone program.  tests/test_cfilter_plan.py compiles and asks it, and also runs it built with -fsanitize=address,undefined.
// TEST INFRASTRUCTURE.  One request per line of stdin:
//   plan   NSAMP IN_SIZE NTAPS DECIM PHASE MAX_RE MAX_IM MIN_IM FORCE -> "nothing nout=0 next=.." |
//                                                            "kernel=.. nout=.. next=.. grid=.. threads=.. run=.. steps=.. runs=.. lds=.."
//   planes IN_SIZE NTAPS DECIM SEED KIND                   -> "planes ok rows=.. steps=.."   (KIND 0: random taps, 1: taps at the sum bound
//                                                            and on the digit seams, stream at its extremes)
//   limits                                                 -> "min_taps8=.. min_taps16=.. max_tap=.. max_run=.. min_run16=.. lds=.. threads=.."
// Every plan is first held to what a plan must hold whatever was asked.  `planes` multiplies the host's digit planes (and, for an
// int16 stream, its two byte planes and the row constants) against a window in plain C++, in the kernels' own arithmetic -- int32
// accumulators, the uint32 recombination -- and compares every row of the tile with the direct complex sum: the CPU proof of the
// operand layout, of the k range, and of the (-128, 0) encoding of a zero sample.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpsiq_cfilter_plan.h"

using namespace gpsiq;

static int show(const FilterPlan &p, int in_size, int ntaps, int decim)
{
    if (!p.launch) return std::printf("nothing nout=%d next=%d\n", p.nout, p.next_phase) < 0;
    const uint64_t window = ((uint64_t) p.run - 1) * (uint64_t) decim + (uint64_t) ntaps;      // samples of a full run's window
    bool ok = p.nout > 0 && p.run >= kFiltThreads && p.run <= kFiltMaxRun && p.run % kFiltThreads == 0 && p.threads == (unsigned) kFiltThreads &&
              p.runs * (uint64_t) p.run >= (uint64_t) p.nout && (p.runs - 1) * (uint64_t) p.run < (uint64_t) p.nout && p.grid >= 1 &&
              p.grid <= kFiltMaxGrid && (uint64_t) p.grid <= p.runs && (p.runs <= kFiltMaxGrid ? p.grid == p.runs : p.grid == kFiltMaxGrid) &&
              p.lds + 64 <= 65536;
    if (p.kernel == kCfiltGeneric) ok = ok && p.steps == 0 && p.lds == 4 * window + 4 * (uint64_t) ntaps && window <= (uint64_t) kFiltGenericWindow;
    else {
        const size_t wbytes = (size_t) filter_mfma_window_bytes(p.run, decim, p.steps);
        ok = ok && p.run % kFiltTileOutputs == 0 && (uint64_t) p.steps * kFiltK >= (uint64_t) (14 * decim + 2 * ntaps) && p.steps <= kFiltMaxSteps &&
             wbytes >= 2 * window && wbytes % 16 == 0 && (p.kernel == kCfiltMfma ? in_size == 1 : p.kernel == kCfiltMfma16 && in_size == 2) &&
             p.lds == (size_t) filter_mfma_plane_bytes(p.steps) + (size_t) in_size * wbytes && p.lds <= (size_t) kFiltMfmaLds;
    }
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("kernel=%d nout=%d next=%d grid=%u threads=%u run=%d steps=%d runs=%" PRIu64 " lds=%zu\n", p.kernel, p.nout, p.next_phase, p.grid,
                       p.threads, p.run, p.steps, p.runs, p.lds) < 0;
}

static uint64_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t) (rng_state >> 33); }
static int rnd_in(int lo, int hi) { return lo + (int) (rnd() % (uint32_t) (hi - lo + 1)); }

// one tile column: 8 outputs from a window of 7 decim + ntaps samples, first output at window sample ntaps - 1
static int planes(int in_size, int ntaps, int decim, uint64_t seed, int kind)
{
    rng_state = seed * 2654435761ULL + 12345;
    std::vector<int16_t> taps(2 * (size_t) ntaps, 0);
    if (kind == 0) {
        const int lim = 65535 / (2 * ntaps);
        for (auto &t : taps) t = (int16_t) rnd_in(-lim, lim);
    } else {                                                          // the sum bound exactly, entries on the digit seams first
        static const int seams[] = {32639, -32639, 127, -128, 128, -127, -129, 255, -256, 256};
        long left = 65535;
        for (size_t i = 0; i < taps.size() && left > 0; ++i) {
            int v = i < 10 ? seams[(i + seed) % 10] : rnd_in(-300, 300);
            if (i + 1 == taps.size() || std::labs((long) v) > left) v = (int) (left > 32639 ? 32639 : left) * ((rnd() & 1) ? 1 : -1);
            if (i % 2 == 0 && v < -32639) v = -32639;
            taps[i] = (int16_t) v;
            left -= std::labs((long) v);
        }
    }
    const CtapStats st = cfilter_tap_stats(taps.data(), ntaps);
    if (st.mag > kCfiltTapSum || !cfilter_mfma_serves(st)) { std::fprintf(stderr, "the test's own taps are outside the matrix path\n"); return 2; }
    const int steps = filter_mfma_steps(ntaps, decim), kbytes = steps * kFiltK, wsamp = 7 * decim + ntaps;
    const int lo = in_size == 1 ? -128 : -32768, hi = in_size == 1 ? 127 : 32767;
    // the window: samples [0, wsamp), the first `zeros` of them the contract's zeros (before the head); past wsamp: padding, zeros
    const int zeros = (int) (seed % 3) * (ntaps / 3);
    std::vector<int32_t> x(2 * (size_t) (kbytes / 2 + 1), 0);
    for (int m = zeros; m < wsamp; ++m)
        for (int c = 0; c < 2; ++c) x[2 * (size_t) m + c] = kind == 1 ? ((rnd() & 1) ? lo : hi) : (rnd() % 8 == 0 ? ((rnd() & 1) ? lo : hi) : rnd_in(lo, hi));
    std::vector<int8_t> pl((size_t) filter_mfma_plane_bytes(steps));
    cfilter_build_planes(taps.data(), ntaps, decim, steps, pl.data());
    const size_t plane = (size_t) steps * kFiltK * 16;
    const auto a_at = [&](int p, int row, int k) { return (int) pl[p * plane + ((size_t) (k / kFiltK) * 64 + (size_t) (16 * ((k % kFiltK) / 16) + row)) * 16 + (size_t) (k % 16)]; };
    int32_t consts[2];
    cfilter_row_consts(taps.data(), ntaps, consts);
    for (int row = 0; row < 16; ++row) {
        const int jj = row >> 1, c = row & 1;
        int64_t want = 0;                                             // the direct sum of the contract
        for (int k = 0; k < ntaps; ++k) {
            const int m = (ntaps - 1) + jj * decim - k;
            const int64_t re = taps[2 * (size_t) k], im = taps[2 * (size_t) k + 1], xi = x[2 * (size_t) m], xq = x[2 * (size_t) m + 1];
            want += c == 0 ? re * xi - im * xq : re * xq + im * xi;
        }
        int64_t rowsum = 0;
        uint32_t got;
        if (in_size == 1) {
            int32_t p0 = 0, p1 = 0;
            for (int k = 0; k < kbytes; ++k) { p0 += a_at(0, row, k) * x[(size_t) k]; p1 += a_at(1, row, k) * x[(size_t) k]; rowsum += a_at(0, row, k) + 256 * a_at(1, row, k); }
            if (std::labs((long) p0) > (1L << 24) || std::labs((long) p1) >= (1L << 17)) { std::fprintf(stderr, "a partial sum leaves its bound\n"); return 1; }
            got = (uint32_t) (p0 + 256 * p1);                         // filter_mfma's int32 recombination
        } else {
            int32_t p00 = 0, pmid = 0, p11 = 0;
            for (int k = 0; k < kbytes; ++k) {
                const int32_t v = x[(size_t) k];                      // a zero of the contract and the padding: (lo' = -128, hi = 0)
                const int hi8 = v >> 8, lo8 = (v & 255) - 128;
                if (256 * hi8 + lo8 + 128 != v || hi8 < -128 || hi8 > 127 || lo8 < -128 || lo8 > 127) { std::fprintf(stderr, "the byte split is not exact\n"); return 1; }
                p00 += a_at(0, row, k) * lo8; pmid += a_at(0, row, k) * hi8 + a_at(1, row, k) * lo8; p11 += a_at(1, row, k) * hi8;
                rowsum += a_at(0, row, k) + 256 * a_at(1, row, k);
            }
            if (std::labs((long) p00) > (1L << 24) || std::labs((long) pmid) > (1L << 24) + (1L << 17) || std::labs((long) p11) >= (1L << 17)) { std::fprintf(stderr, "a partial sum leaves its bound\n"); return 1; }
            got = (uint32_t) p00 + ((uint32_t) pmid << 8) + ((uint32_t) p11 << 16) + (uint32_t) consts[c];      // cfilter_mfma16's, modulo 2^32
            if (128 * rowsum != consts[c]) { std::fprintf(stderr, "row %d: constant %d is not 128 x the row's sum %lld\n", row, consts[c], (long long) rowsum); return 1; }
        }
        if (want >= (int64_t) 1 << 31 || want < -((int64_t) 1 << 31) || (int32_t) got != (int32_t) want) {
            std::fprintf(stderr, "row %d: planes give %d, the direct sum %lld\n", row, (int32_t) got, (long long) want);
            return 1;
        }
    }
    return std::printf("planes ok rows=16 steps=%d\n", steps) < 0;
}

int main()
{
    char what[16];
    long long a, b, c, d, e, f, g, h, i;
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "plan")) {
            if (std::scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld", &a, &b, &c, &d, &e, &f, &g, &h, &i) != 9) return 2;
            if (a < 0 || (b != 1 && b != 2) || c < 1 || c > kFiltMaxTaps || d < 1 || d > kFiltMaxDecim || e < 0 || e >= d) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            CtapStats st;
            st.max_re = (int) f; st.max_im = (int) g; st.min_im = (int) h;
            if (show(plan_cfilter((int) a, (int) b, (int) c, (int) d, (int) e, st, (int) i), (int) b, (int) c, (int) d)) return 1;
        } else if (!std::strcmp(what, "planes")) {
            if (std::scanf("%lld %lld %lld %lld %lld", &a, &b, &c, &d, &e) != 5) return 2;
            if ((a != 1 && a != 2) || b < 1 || b > kFiltMaxTaps || c < 1 || c > kFiltMaxDecim) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (int rc = planes((int) a, (int) b, (int) c, (uint64_t) d, (int) e)) return rc;
        } else if (!std::strcmp(what, "limits")) {
            std::printf("min_taps8=%d min_taps16=%d max_tap=%d max_run=%d min_run16=%d lds=%d threads=%d\n", kCfiltMfmaMinTaps8, kCfiltMfmaMinTaps16,
                        kFiltMfmaMaxTap, kFiltMaxRun, kCfiltMinRun16, kFiltMfmaLds, kFiltThreads);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
