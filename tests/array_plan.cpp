// array_plan.cpp -- csrc/gpsiq_array_plan.h, the header gpsiq_array_cov and gpsiq_array_combine plan with and turn the device scratch
// into the covariance with, as a stand-alone program.  tests/test_array_plan.py compiles and asks it, and also runs it built with
// -fsanitize=address,undefined.  TEST INFRASTRUCTURE.  One request per line of stdin:
//   cov     NELEM NSAMP IN_SIZE FORCE   -> "nothing" | "kernel=.. grid=.. threads=.. run=.. runs=.. steps=.."
//   combine NSAMP OUT_SIZE DST_LOW4     -> "nothing" | "grid=.. threads=.. lead=.. slots=.."
//   gram    NELEM NSAMP SEED KIND       -> "gram ok peak=.. flushes=.."   (KIND 0: random bytes, 1: every byte -128, 2: extremes at random)
//   limits                              -> "max_elem=.. k=.. flush=.. min_run=.. max_grid=.. gen_run=.. gen_grid=.. chunk=.. min_elem=.. threads=.. comb_grid=.."
// Every plan is first held to what a plan must hold whatever was asked.  `gram` multiplies ONE wave's k-steps out in plain C++ in the
// matrix kernel's own arithmetic -- the 16 rows I_0, Q_0, ... of 64 bytes a k-step, rows of absent elements zero, the span's tail
// padded with zeros, int32 entries added into int64 every kArrFlushSteps k-steps -- holds every int32 entry to its bound, and
// compares array_scratch_to_cov of the tile with the direct complex sums: the CPU proof of the Gram-to-R mapping and the flush bound.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpsiq_array_plan.h"

using namespace gpsiq;

static int show_cov(const ArrayCovPlan &p, int nsamp)
{
    if (!p.launch) return std::printf("nothing\n") < 0;
    bool ok = p.threads == (unsigned) kArrThreads && p.grid >= 1 && p.runs >= 1 && (p.runs - 1) * p.run < (p.kernel == kArrMfma ? p.steps : (uint64_t) nsamp);
    if (p.kernel == kArrMfma)
        ok = ok && p.steps * kArrK >= (uint64_t) nsamp && (p.steps - 1) * kArrK < (uint64_t) nsamp && p.run % kArrWaves == 0 && p.run >= (uint64_t) kArrMinRunSteps &&
             p.grid == p.runs && p.grid <= kArrMaxGrid && p.runs * p.run >= p.steps;
    else
        ok = ok && p.steps == 0 && p.run == (uint64_t) kArrGenRun && p.runs * p.run >= (uint64_t) nsamp && p.grid <= kArrGenMaxGrid && (uint64_t) p.grid <= p.runs;
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("kernel=%d grid=%u threads=%u run=%" PRIu64 " runs=%" PRIu64 " steps=%" PRIu64 "\n", p.kernel, p.grid, p.threads, p.run, p.runs, p.steps) < 0;
}

static int show_combine(const ArrayCombinePlan &p, int nsamp, int out_size)
{
    if (!p.launch) return std::printf("nothing\n") < 0;
    const uint64_t S = (uint64_t) array_slot_samples(out_size);
    const bool ok = p.threads == (unsigned) kArrThreads && p.lead >= 0 && (uint64_t) p.lead < S && p.slots * S >= (uint64_t) nsamp + (uint64_t) p.lead &&
                    (p.slots - 1) * S < (uint64_t) nsamp + (uint64_t) p.lead && p.grid >= 1 && p.grid <= kArrCombMaxGrid &&
                    (uint64_t) (p.grid - 1) * kArrThreads < p.slots;
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("grid=%u threads=%u lead=%d slots=%" PRIu64 "\n", p.grid, p.threads, p.lead, p.slots) < 0;
}

static uint64_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t) (rng_state >> 33); }

static int gram(int nelem, int nsamp, uint64_t seed, int kind)
{
    rng_state = seed * 2654435761ULL + 977;
    std::vector<int8_t> x((size_t) nelem * 2 * (size_t) nsamp);       // x[e][n][c]
    for (auto &v : x) v = kind == 1 ? (int8_t) -128 : kind == 2 ? ((rnd() & 1) ? (int8_t) -128 : (int8_t) 127) : (int8_t) (int) (rnd() % 256 - 128);
    const uint64_t steps = ((uint64_t) nsamp + kArrK - 1) / kArrK;
    int64_t sum[kArrGramWords] = {0}, peak = 0;
    int32_t acc[kArrGramWords] = {0};
    int pending = 0, flushes = 0;
    for (uint64_t s = 0; s < steps; ++s) {
        int8_t rows[kArrRows][kArrK];
        std::memset(rows, 0, sizeof rows);                            // rows of absent elements, and the tail past the span
        for (int e = 0; e < nelem; ++e)
            for (int k = 0; k < kArrK; ++k) {
                const uint64_t n = s * kArrK + (uint64_t) k;
                if (n >= (uint64_t) nsamp) break;
                for (int c = 0; c < 2; ++c) rows[2 * e + c][k] = x[((size_t) e * (size_t) nsamp + (size_t) n) * 2 + (size_t) c];
            }
        for (int i = 0; i < kArrRows; ++i)
            for (int j = 0; j < kArrRows; ++j) {
                int64_t d = acc[i * kArrRows + j];
                for (int k = 0; k < kArrK; ++k) d += (int32_t) rows[i][k] * (int32_t) rows[j][k];
                if (d > INT32_MAX || d < INT32_MIN) { std::fprintf(stderr, "entry (%d, %d) leaves int32 at k-step %" PRIu64 "\n", i, j, s); return 1; }
                acc[i * kArrRows + j] = (int32_t) d;
                if (std::llabs((long long) d) > peak) peak = std::llabs((long long) d);
            }
        if (++pending == kArrFlushSteps) {
            for (int w = 0; w < kArrGramWords; ++w) { sum[w] += acc[w]; acc[w] = 0; }
            pending = 0;
            ++flushes;
        }
    }
    for (int w = 0; w < kArrGramWords; ++w) sum[w] += acc[w];
    std::vector<int64_t> cov((size_t) 2 * nelem * nelem);
    array_scratch_to_cov(kArrMfma, sum, nelem, cov.data());
    for (int a = 0; a < nelem; ++a)
        for (int b = 0; b < nelem; ++b) {
            int64_t re = 0, im = 0;
            for (int n = 0; n < nsamp; ++n) {
                const int64_t ia = x[((size_t) a * nsamp + n) * 2], qa = x[((size_t) a * nsamp + n) * 2 + 1], ib = x[((size_t) b * nsamp + n) * 2], qb = x[((size_t) b * nsamp + n) * 2 + 1];
                re += ia * ib + qa * qb;
                im += qa * ib - ia * qb;
            }
            if (cov[2 * ((size_t) a * nelem + b)] != re || cov[2 * ((size_t) a * nelem + b) + 1] != im) {
                std::fprintf(stderr, "R[%d][%d]: the tile gives (%lld, %lld), the direct sum (%lld, %lld)\n", a, b, (long long) cov[2 * ((size_t) a * nelem + b)],
                             (long long) cov[2 * ((size_t) a * nelem + b) + 1], (long long) re, (long long) im);
                return 1;
            }
        }
    for (int i = 2 * nelem; i < kArrRows; ++i)
        for (int j = 0; j < kArrRows; ++j)
            if (sum[i * kArrRows + j] || sum[j * kArrRows + i]) { std::fprintf(stderr, "an absent row is not zero\n"); return 1; }
    return std::printf("gram ok peak=%" PRId64 " flushes=%d\n", peak, flushes) < 0;
}

int main()
{
    char what[16];
    long long a, b, c, d;
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "cov")) {
            if (std::scanf("%lld %lld %lld %lld", &a, &b, &c, &d) != 4) return 2;
            if (a < 1 || a > kArrMaxElem || b < 0 || b > INT32_MAX || (c != 1 && c != 2)) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (show_cov(plan_array_cov((int) a, (int) b, (int) c, (int) d), (int) b)) return 1;
        } else if (!std::strcmp(what, "combine")) {
            if (std::scanf("%lld %lld %lld", &a, &b, &c) != 3) return 2;
            if (a < 0 || a > INT32_MAX || (b != 1 && b != 2) || c < 0 || c > 15 || (c & 3)) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (show_combine(plan_array_combine((int) a, (int) b, (unsigned) c), (int) a, (int) b)) return 1;
        } else if (!std::strcmp(what, "gram")) {
            if (std::scanf("%lld %lld %lld %lld", &a, &b, &c, &d) != 4) return 2;
            if (a < 1 || a > kArrMaxElem || b < 1 || b > (1 << 20)) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (int rc = gram((int) a, (int) b, (uint64_t) c, (int) d)) return rc;
        } else if (!std::strcmp(what, "limits")) {
            std::printf("max_elem=%d k=%d flush=%d min_run=%d max_grid=%u gen_run=%d gen_grid=%u chunk=%d min_elem=%d threads=%d comb_grid=%u\n", kArrMaxElem, kArrK,
                        kArrFlushSteps, kArrMinRunSteps, kArrMaxGrid, kArrGenRun, kArrGenMaxGrid, kArrChunk, kArrMfmaMinElem, kArrThreads, kArrCombMaxGrid);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
