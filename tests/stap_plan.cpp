// stap_plan.cpp -- csrc/gpsiq_stap_plan.h, the header gpsiq_stap_cov and gpsiq_stap_combine plan with and turn the device scratch into
// the covariance with, as a stand-alone program.  tests/test_stap_plan.py compiles and asks it, and also runs it built with
// -fsanitize=address,undefined.  TEST INFRASTRUCTURE.  One request per line of stdin:
//   cov     NELEM NTAPS NSAMP IN_SIZE FORCE   -> "nothing" | "kernel=.. groups=.. grid=.. threads=.. run=.. runs=.. steps=.."
//   combine NSAMP OUT_SIZE DST_LOW4           -> "nothing" | "grid=.. threads=.. lead=.. slots=.."
//   gram    NELEM NTAPS NSAMP SEED KIND HEADS -> "gram ok peak=.. flushes=.. tiles=.."
//           (KIND 0: random bytes, 1: every byte -128, 2: extremes at random; HEADS 0: none, 1: every element, 2: every other element)
//   limits                                    -> "max_elem=.. max_taps=.. max_rows=.. k=.. flush=.. min_run=.. max_grid=.. gen_run=.. ..."
// Every plan is first held to what a plan must hold whatever was asked.  `gram` multiplies ONE wave's k-steps out in plain C++ in the
// matrix kernel's own arithmetic and layout: the 64 lanes' 16 bytes of every row group (component lane & 1 of row 8 g + ((lane & 15)
// >> 1), element k / ntaps, tap k % ntaps, samples 64 s + 16 (lane >> 4) + i - tap, from the head or zero before the span, and zero
// where 64 s + 16 (lane >> 4) + i is past the span: a row ends with the span, tap samples before its stream does), the tiles (g, h),
// g >= h, by an instruction modelled on its measured register map -- A lane l feeds row l & 15, B lane l feeds column l & 15, D(row, col) is register row & 3 of lane col + 16 (row >> 2) -- int32 entries added into int64 every
// kStapFlushSteps k-steps, the kernel's own way from a lane's registers to the scratch, and stap_scratch_to_cov with its mirror.  It
// holds every int32 entry to its bound and compares with the direct complex sums of the shifted rows: random data is not symmetric
// under an exchange of the operands, so a tile read the wrong way round, or a tap counted forwards, cannot pass.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpsiq_stap_plan.h"

using namespace gpsiq;

static int show_cov(const StapCovPlan &p, int rows, int nsamp)
{
    if (!p.launch) return std::printf("nothing\n") < 0;
    bool ok = p.threads == (unsigned) kStapThreads && p.grid >= 1 && p.runs >= 1 && (p.runs - 1) * p.run < (p.kernel == kStapMfma ? p.steps : (uint64_t) nsamp);
    if (p.kernel == kStapMfma)
        ok = ok && p.steps * kStapK >= (uint64_t) nsamp && (p.steps - 1) * kStapK < (uint64_t) nsamp && p.run % kStapWaves == 0 && p.run >= (uint64_t) kStapMinRunSteps &&
             p.grid == p.runs && p.grid <= kStapMaxGrid && p.runs * p.run >= p.steps && p.groups >= 1 && p.groups <= kStapMaxGroups && 8 * p.groups >= rows &&
             8 * (p.groups - 1) < rows;
    else
        ok = ok && p.steps == 0 && p.groups == 0 && p.run == (uint64_t) kStapGenRun && p.runs * p.run >= (uint64_t) nsamp && p.grid <= kStapGenMaxGrid &&
             (uint64_t) p.grid <= p.runs;
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("kernel=%d groups=%d grid=%u threads=%u run=%" PRIu64 " runs=%" PRIu64 " steps=%" PRIu64 "\n", p.kernel, p.groups, p.grid, p.threads, p.run,
                       p.runs, p.steps) < 0;
}

static int show_combine(const StapCombinePlan &p, int nsamp, int out_size)
{
    if (!p.launch) return std::printf("nothing\n") < 0;
    const uint64_t S = (uint64_t) stap_slot_samples(out_size);
    const bool ok = p.threads == (unsigned) kStapThreads && p.lead >= 0 && (uint64_t) p.lead < S && p.slots * S >= (uint64_t) nsamp + (uint64_t) p.lead &&
                    (p.slots - 1) * S < (uint64_t) nsamp + (uint64_t) p.lead && p.grid >= 1 && p.grid <= kStapCombMaxGrid &&
                    (uint64_t) (p.grid - 1) * kStapThreads < p.slots;
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("grid=%u threads=%u lead=%d slots=%" PRIu64 "\n", p.grid, p.threads, p.lead, p.slots) < 0;
}

static uint64_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t) (rng_state >> 33); }

struct Scene {
    int nelem, ntaps, nsamp;
    std::vector<int8_t> x;        // x[e][n][c]
    std::vector<int8_t> head;     // head[e][m][c], ntaps - 1 samples
    bool has_head[kStapMaxElem];
    // x_e(m) of the contract, component c
    int at(int e, int64_t m, int c) const
    {
        if (m >= (int64_t) nsamp) return 0;
        if (m >= 0) return x[((size_t) e * (size_t) nsamp + (size_t) m) * 2 + (size_t) c];
        if (!has_head[e] || m < -(int64_t) (ntaps - 1)) return 0;
        return head[((size_t) e * (size_t) (ntaps - 1) + (size_t) (ntaps - 1 + m)) * 2 + (size_t) c];
    }
};

static int gram(int nelem, int ntaps, int nsamp, uint64_t seed, int kind, int heads)
{
    rng_state = seed * 2654435761ULL + 977;
    const auto byte = [&]() { return kind == 1 ? (int8_t) -128 : kind == 2 ? ((rnd() & 1) ? (int8_t) -128 : (int8_t) 127) : (int8_t) (int) (rnd() % 256 - 128); };
    Scene sc{nelem, ntaps, nsamp, std::vector<int8_t>((size_t) nelem * 2 * (size_t) nsamp), std::vector<int8_t>((size_t) nelem * 2 * (size_t) (ntaps - 1) + 1), {}};
    for (auto &v : sc.x) v = byte();
    for (auto &v : sc.head) v = byte();
    for (int e = 0; e < kStapMaxElem; ++e) sc.has_head[e] = heads == 1 || (heads == 2 && (e & 1));
    const int rows = nelem * ntaps, G = stap_groups(rows), T = stap_tiles(G);
    const uint64_t steps = ((uint64_t) nsamp + kStapK - 1) / kStapK;
    std::vector<int64_t> scratch(kStapGramWords, 0);
    std::vector<int64_t> sum((size_t) T * 64 * 4, 0);                  // a wave's registers: [tile][lane][register]
    std::vector<int32_t> acc((size_t) T * 64 * 4, 0);
    int64_t peak = 0;
    int pending = 0, flushes = 0;
    for (uint64_t s = 0; s < steps; ++s) {
        int8_t v[kStapMaxGroups][64][kStapLaneSamples];                // what lane l holds for group g
        for (int g = 0; g < G; ++g)
            for (int l = 0; l < 64; ++l) {
                const int row = l & 15, q = l >> 4, k = 8 * g + (row >> 1), c = row & 1;
                for (int i = 0; i < kStapLaneSamples; ++i) {
                    const int64_t n = (int64_t) (s * kStapK) + kStapLaneSamples * q + i;     // the row's own time: it ends with the span
                    v[g][l][i] = k < rows && n < (int64_t) nsamp ? (int8_t) sc.at(k / ntaps, n - k % ntaps, c) : (int8_t) 0;
                }
            }
        int t = 0;
        for (int g = 0; g < G; ++g)
            for (int h = 0; h <= g; ++h, ++t)
                for (int i = 0; i < kStapTile; ++i)                    // D(i, j) += sum over k of A(i, k) B(k, j): A lanes i + 16 q, B lanes j + 16 q
                    for (int j = 0; j < kStapTile; ++j) {
                        int32_t &d32 = acc[((size_t) t * 64 + (size_t) (j + 16 * (i >> 2))) * 4 + (size_t) (i & 3)];
                        int64_t d = d32;
                        for (int q = 0; q < 4; ++q)
                            for (int b = 0; b < kStapLaneSamples; ++b) d += (int32_t) v[g][i + 16 * q][b] * (int32_t) v[h][j + 16 * q][b];
                        if (d > INT32_MAX || d < INT32_MIN) { std::fprintf(stderr, "tile (%d, %d) entry (%d, %d) leaves int32 at k-step %" PRIu64 "\n", g, h, i, j, s); return 1; }
                        d32 = (int32_t) d;
                        if (std::llabs((long long) d) > peak) peak = std::llabs((long long) d);
                    }
        if (++pending == kStapFlushSteps) {
            for (size_t w = 0; w < acc.size(); ++w) { sum[w] += acc[w]; acc[w] = 0; }
            pending = 0;
            ++flushes;
        }
    }
    {
        int t = 0;                                                     // the kernel's way out: register r of lane l of tile (g, h) is Gm[16 g + 4 (l >> 4) + r][16 h + (l & 15)]
        for (int g = 0; g < G; ++g)
            for (int h = 0; h <= g; ++h, ++t)
                for (int l = 0; l < 64; ++l)
                    for (int r = 0; r < 4; ++r) {
                        const size_t w = ((size_t) t * 64 + (size_t) l) * 4 + (size_t) r;
                        scratch[(size_t) (kStapTile * g + 4 * (l >> 4) + r) * kStapRealRows + (size_t) (kStapTile * h + (l & 15))] += sum[w] + acc[w];
                    }
    }
    std::vector<int64_t> cov((size_t) 2 * rows * rows);
    stap_scratch_to_cov(kStapMfma, scratch.data(), rows, cov.data());
    for (int k = 0; k < rows; ++k)
        for (int l = 0; l < rows; ++l) {
            int64_t re = 0, im = 0;
            for (int n = 0; n < nsamp; ++n) {
                const int64_t ia = sc.at(k / ntaps, n - k % ntaps, 0), qa = sc.at(k / ntaps, n - k % ntaps, 1);
                const int64_t ib = sc.at(l / ntaps, n - l % ntaps, 0), qb = sc.at(l / ntaps, n - l % ntaps, 1);
                re += ia * ib + qa * qb;
                im += qa * ib - ia * qb;
            }
            const int64_t *got = &cov[2 * ((size_t) k * rows + l)];
            if (got[0] != re || got[1] != im) {
                std::fprintf(stderr, "R[%d][%d]: the tiles give (%lld, %lld), the direct sum (%lld, %lld)\n", k, l, (long long) got[0], (long long) got[1], (long long) re,
                             (long long) im);
                return 1;
            }
        }
    for (int i = 2 * rows; i < kStapTile * G; ++i)
        for (int j = 0; j < kStapRealRows; ++j)
            if (stap_gram_entry(scratch.data(), i, j)) { std::fprintf(stderr, "an absent row is not zero\n"); return 1; }
    for (int g = 0; g < kStapMaxGroups; ++g)                           // the upper tiles and the groups beyond G are never written
        for (int h = 0; h < kStapMaxGroups; ++h)
            if (h > g || g >= G)
                for (int i = 0; i < kStapTile; ++i)
                    for (int j = 0; j < kStapTile; ++j)
                        if (scratch[(size_t) (kStapTile * g + i) * kStapRealRows + (size_t) (kStapTile * h + j)]) { std::fprintf(stderr, "a tile that is not computed is not zero\n"); return 1; }
    return std::printf("gram ok peak=%" PRId64 " flushes=%d tiles=%d\n", peak, flushes, T) < 0;
}

int main()
{
    char what[16];
    long long a, b, c, d, e, f;
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "cov")) {
            if (std::scanf("%lld %lld %lld %lld %lld", &a, &b, &c, &d, &e) != 5) return 2;
            if (a < 1 || a > kStapMaxElem || b < 1 || b > kStapMaxTaps || a * b > kStapMaxRows || c < 0 || c > INT32_MAX || (d != 1 && d != 2)) {
                std::fprintf(stderr, "request outside the ranges\n");
                return 2;
            }
            if (show_cov(plan_stap_cov((int) a, (int) b, (int) c, (int) d, (int) e), (int) (a * b), (int) c)) return 1;
        } else if (!std::strcmp(what, "combine")) {
            if (std::scanf("%lld %lld %lld", &a, &b, &c) != 3) return 2;
            if (a < 0 || a > INT32_MAX || (b != 1 && b != 2) || c < 0 || c > 15 || (c & 3)) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (show_combine(plan_stap_combine((int) a, (int) b, (unsigned) c), (int) a, (int) b)) return 1;
        } else if (!std::strcmp(what, "gram")) {
            if (std::scanf("%lld %lld %lld %lld %lld %lld", &a, &b, &c, &d, &e, &f) != 6) return 2;
            if (a < 1 || a > kStapMaxElem || b < 1 || b > kStapMaxTaps || a * b > kStapMaxRows || c < 1 || c > (1 << 20) || e < 0 || e > 2 || f < 0 || f > 2) {
                std::fprintf(stderr, "request outside the ranges\n");
                return 2;
            }
            if (int rc = gram((int) a, (int) b, (int) c, (uint64_t) d, (int) e, (int) f)) return rc;
        } else if (!std::strcmp(what, "limits")) {
            std::printf("max_elem=%d max_taps=%d max_rows=%d k=%d flush=%d min_run=%d max_grid=%u gen_run=%d gen_grid=%u chunk=%d min_rows=%d threads=%d comb_grid=%u gram_words=%d\n",
                        kStapMaxElem, kStapMaxTaps, kStapMaxRows, kStapK, kStapFlushSteps, kStapMinRunSteps, kStapMaxGrid, kStapGenRun, kStapGenMaxGrid, kStapChunk,
                        kStapMfmaMinRows, kStapThreads, kStapCombMaxGrid, kStapGramWords);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
