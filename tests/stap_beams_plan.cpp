// stap_beams_plan.cpp -- csrc/gpsiq_stap_beams_plan.h, the header gpsiq_stap_beams plans with and builds the matrix kernel's operand
// with, as a stand-alone program.  tests/test_stap_beams_plan.py compiles and asks it, and also runs it built with
// -fsanitize=address,undefined.  TEST INFRASTRUCTURE.  One request per line of stdin:
//   plan   NELEM NTAPS NBEAMS NSAMP IN_SIZE OUT_SIZE MAX_ENTRY FORCE -> "nothing" | "kernel=.. padded=.. grid=.. threads=.. run=.. runs=.. can=.."
//   split  LO HI                                             -> "split ok planes=.. generic=.."   every value of LO .. HI as an entry
//   planes NELEM NTAPS NBEAMS SEED KIND                      -> "planes ok"                        (KIND 0: random weights, 1: at the bound)
//   tile   NELEM NTAPS NBEAMS IN_SIZE OUT_SIZE NSAMP SEED KIND HEADS -> "tile ok peak=.. acc=.."
//          (KIND 0: random data and weights, 1: every sample at the format's minimum and weights at the bound with random signs,
//           2: extremes at random and weights at the bound; HEADS 0: none, 1: every element, 2: every other element; NSAMP <= a chunk)
//   minrows IN_SIZE NBEAMS                                   -> "rows=.."   the padded rows from which the matrix kernel is the default
//   limits                                                   -> "max_beams=.. max_entry=.. chunk8=.. chunk16=.. ..."
// `split` holds every entry either to two signed bytes that multiply out, d0 + 256 d1, or to the planner's refusal of the matrix
// kernel.  `planes` multiplies both planes of every (row, k) out against the weights, read back through the k-byte order written out
// here once more, and sums the row constants.  `tile` models ONE chunk of the matrix kernel in plain C++: the staged bytes (int16 as the
// planes lo' and hi, a zero of the contract as (-128, 0)), operand B by the k-byte order, operand A from the planes in fragment order,
// the instruction by its measured register map -- A lane l feeds row l & 15 with bytes k = 16 (l >> 4) + j, B lane l feeds column
// l & 15, D(row, col) is register row & 3 of lane col + 16 (row >> 2) -- the recombination modulo 2^32, and holds every plane product to
// its bound and every sum to the direct complex sum.  Random weights differ from beam to beam and from re to im, so an exchange of the
// operands, of two beams or of the components cannot pass.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpsiq_stap_beams_plan.h"

using namespace gpsiq;

static uint64_t rng_state;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t) (rng_state >> 33); }

static int show_plan(const BeamsPlan &p, int nelem, int ntaps, int nsamp, int out_size, int max_entry)
{
    if (!p.launch) return std::printf("nothing\n") < 0;
    const bool can = beams_mfma_serves(nelem, ntaps, max_entry);
    bool ok = p.threads == (unsigned) kBeamsThreads && p.grid >= 1 && p.runs >= 1 && (uint64_t) p.grid <= p.runs && p.run >= 1 &&
              p.runs * (uint64_t) p.run >= (uint64_t) nsamp && (p.runs - 1) * (uint64_t) p.run < (uint64_t) nsamp;
    if (p.kernel == kBeamsMfma)
        ok = ok && can && p.padded >= ntaps && p.padded < 2 * ntaps && nelem * p.padded <= kStapMaxRows && nelem <= beams_max_elem(p.padded) &&
             (p.padded & (p.padded - 1)) == 0 && p.run == beams_chunk_samples(out_size) && p.grid <= kBeamsMaxGrid;
    else
        ok = ok && p.kernel == kBeamsGeneric && p.padded == 0 && p.run == kBeamsThreads * beams_lane_samples(out_size) && p.grid <= kBeamsGenMaxGrid;
    if (!ok) { std::fprintf(stderr, "plan does not hold its own invariants\n"); return 1; }
    return std::printf("kernel=%d padded=%d grid=%u threads=%u run=%d runs=%" PRIu64 " can=%d\n", p.kernel, p.padded, p.grid, p.threads, p.run, p.runs, (int) can) < 0;
}

static int split(int lo, int hi)
{
    long planes = 0, generic = 0;
    for (int v = lo; v <= hi; ++v) {
        // the entry as the one weight (re = v, im = 0) of one element with one tap presents it, and as -im of (0, -v) where that is an int16
        int16_t w[2] = {(int16_t) v, 0};
        const BeamsStats st = beams_weight_stats(w, 1);
        if (st.max_entry != (v > 0 ? v : 0)) { std::fprintf(stderr, "max_entry of %d is %d\n", v, st.max_entry); return 1; }
        if (!beams_mfma_serves(1, 1, st.max_entry)) {
            if (v <= kBeamsMaxEntry) { std::fprintf(stderr, "%d is refused\n", v); return 1; }
            ++generic;
            continue;
        }
        uint32_t coef[kBeamsCoefDwords];
        beams_build_coef(w, 1, 1, 1, 1, coef);
        const int8_t *pl = reinterpret_cast<const int8_t *>(coef);
        // row 0, k 0 (re at the byte of I) and row 1, k 1 (re at the byte of Q): lanes 0 and 1 of group 0
        const int d0 = pl[0], d1 = pl[kBeamsPlaneBytes], e0 = pl[16 + 1], e1 = pl[kBeamsPlaneBytes + 16 + 1];
        if (d0 + 256 * d1 != v || e0 + 256 * e1 != v) { std::fprintf(stderr, "%d splits into %d + 256 * %d\n", v, d0, d1); return 1; }
        ++planes;
    }
    return std::printf("split ok planes=%ld generic=%ld\n", planes, generic) < 0;
}

// weights [nbeams][nelem][ntaps][2] inside the bound and the digit planes' range; at_bound: magnitudes that sum to the bound (as far as
// the planes' range allows), signs at random
static std::vector<int16_t> make_weights(int nelem, int ntaps, int nbeams, bool at_bound)
{
    const int rows = nelem * ntaps;
    std::vector<int16_t> w((size_t) 2 * nbeams * rows);
    for (int b = 0; b < nbeams; ++b) {
        int each = (int) (kStapWeightSum / (2 * rows));
        if (each > kBeamsMaxEntry) each = kBeamsMaxEntry;
        long left = kStapWeightSum - (long) each * 2 * rows;
        for (int k = 0; k < 2 * rows; ++k) {
            int mag = at_bound ? each : (int) (rnd() % (uint32_t) (each + 1));
            if (at_bound && left > 0 && mag < kBeamsMaxEntry) { const long add = left < kBeamsMaxEntry - mag ? left : kBeamsMaxEntry - mag; mag += (int) add; left -= add; }
            w[(size_t) 2 * b * rows + k] = (int16_t) ((rnd() & 1) ? -mag : mag);
        }
    }
    return w;
}

static int planes(int nelem, int ntaps, int nbeams, uint64_t seed, int kind)
{
    rng_state = seed * 2654435761ULL + 4242;
    const int tp = beams_padded_taps(nelem, ntaps);
    if (!tp) { std::fprintf(stderr, "the shape does not pad into %d rows\n", kStapMaxRows); return 2; }
    const std::vector<int16_t> w = make_weights(nelem, ntaps, nbeams, kind == 1);
    uint32_t coef[kBeamsCoefDwords];
    beams_build_coef(w.data(), nelem, ntaps, nbeams, tp, coef);
    const int8_t *pl = reinterpret_cast<const int8_t *>(coef);
    const int32_t *consts = reinterpret_cast<const int32_t *>(coef + kBeamsConstAt);
    std::vector<int> want((size_t) kBeamsRows * kBeamsK, 0);           // the operand written out from the contract's sums
    for (int b = 0; b < nbeams; ++b)
        for (int e = 0; e < nelem; ++e)
            for (int t = 0; t < ntaps; ++t) {
                const int re = w[2 * (((size_t) b * nelem + e) * ntaps + t)], im = w[2 * (((size_t) b * nelem + e) * ntaps + t) + 1];
                const int ki = 2 * tp * e + 2 * (tp - 1 - t), kq = ki + 1;      // the bytes of I and Q of x_e(n - t) in the window
                want[(size_t) (2 * b) * kBeamsK + ki] = re;      want[(size_t) (2 * b) * kBeamsK + kq] = -im;       // accI = re I - im Q
                want[(size_t) (2 * b + 1) * kBeamsK + ki] = im;  want[(size_t) (2 * b + 1) * kBeamsK + kq] = re;    // accQ = im I + re Q
            }
    for (int row = 0; row < kBeamsRows; ++row) {
        long sum = 0;
        for (int k = 0; k < kBeamsK; ++k) {
            const size_t at = (size_t) (16 * (k / 16) + row) * 16 + (size_t) (k % 16);      // lane (row, group k / 16), byte k % 16
            const int got = pl[at] + 256 * pl[kBeamsPlaneBytes + at];
            if (got != want[(size_t) row * kBeamsK + k] || beams_kbyte(tp, k / (2 * tp), tp - 1 - (k % (2 * tp)) / 2, k & 1) != k) {
                std::fprintf(stderr, "A(%d, %d): the planes give %d, the weights %d\n", row, k, got, want[(size_t) row * kBeamsK + k]);
                return 1;
            }
            sum += got;
        }
        if (consts[row] != 128 * sum) { std::fprintf(stderr, "row constant %d\n", row); return 1; }
    }
    for (int b = 0; b < kBeamsMax; ++b)
        for (int r = 0; r < kStapMaxRows; ++r) {
            const uint32_t got = coef[kBeamsWeightsAt + b * kStapMaxRows + r];
            const uint32_t exp = b < nbeams && r < nelem * ntaps
                                     ? (uint32_t) (uint16_t) w[2 * ((size_t) b * nelem * ntaps + r)] | ((uint32_t) (uint16_t) w[2 * ((size_t) b * nelem * ntaps + r) + 1] << 16)
                                     : 0u;
            if (got != exp) { std::fprintf(stderr, "weight dword (%d, %d)\n", b, r); return 1; }
        }
    return std::printf("planes ok\n") < 0;
}

struct Scene {
    int nelem, ntaps, nsamp, size;
    std::vector<int16_t> x, head;      // x[e][n][c]; head[e][m][c], ntaps - 1 samples
    bool has_head[kStapMaxElem];
    int at(int e, int64_t m, int c) const      // x_e(m) of the contract
    {
        if (m >= (int64_t) nsamp) return 0;
        if (m >= 0) return x[((size_t) e * (size_t) nsamp + (size_t) m) * 2 + (size_t) c];
        if (!has_head[e] || m < -(int64_t) (ntaps - 1)) return 0;
        return head[((size_t) e * (size_t) (ntaps - 1) + (size_t) (ntaps - 1 + m)) * 2 + (size_t) c];
    }
};

static int tile(int nelem, int ntaps, int nbeams, int in_size, int out_size, int nsamp, uint64_t seed, int kind, int heads)
{
    rng_state = seed * 2654435761ULL + 1717;
    const int tp = beams_padded_taps(nelem, ntaps);
    if (!tp) { std::fprintf(stderr, "the shape does not pad into %d rows\n", kStapMaxRows); return 2; }
    const int lo = in_size == 1 ? -128 : -32768, hi = in_size == 1 ? 127 : 32767;
    const auto value = [&]() { return (int16_t) (kind == 1 ? lo : kind == 2 ? ((rnd() & 1) ? lo : hi) : (int) (rnd() % (uint32_t) (hi - lo + 1)) + lo); };
    Scene sc{nelem, ntaps, nsamp, in_size, std::vector<int16_t>((size_t) nelem * 2 * (size_t) nsamp), std::vector<int16_t>((size_t) nelem * 2 * (size_t) (ntaps - 1) + 1), {}};
    for (auto &v : sc.x) v = value();
    for (auto &v : sc.head) v = value();
    for (int e = 0; e < kStapMaxElem; ++e) sc.has_head[e] = heads == 1 || (heads == 2 && (e & 1));
    const std::vector<int16_t> w = make_weights(nelem, ntaps, nbeams, kind != 0);
    uint32_t coef[kBeamsCoefDwords];
    beams_build_coef(w.data(), nelem, ntaps, nbeams, tp, coef);
    const int8_t *pl = reinterpret_cast<const int8_t *>(coef);
    const int32_t *consts = reinterpret_cast<const int32_t *>(coef + kBeamsConstAt);
    const int S = beams_lane_samples(out_size), TILE = beams_tile_samples(out_size), CHUNK = beams_chunk_samples(out_size), planes_in = in_size;
    if (nsamp > CHUNK) { std::fprintf(stderr, "more than a chunk\n"); return 2; }
    // the staged byte of plane pl_ of sample m, component c: the stream's own byte (int8), lo' or hi (int16)
    const auto staged = [&](int pl_, int e, int64_t m, int c) -> int {
        const int v = sc.at(e, m, c);
        if (in_size == 1) return v;
        return pl_ == 0 ? (v & 255) - 128 : v >> 8;
    };
    int64_t peak = 0, peak_acc = 0;
    for (int wave = 0; wave < kBeamsWaves; ++wave)
        for (int j = 0; j < S; ++j) {
            int8_t bop[2][64][16];                                     // operand B of step j: [plane][lane][byte]
            for (int l = 0; l < 64; ++l) {
                const int col = l & 15, g = l >> 4;
                const int64_t n = (int64_t) wave * TILE + (int64_t) S * col + j;
                for (int kb = 0; kb < 16; ++kb) {
                    const int k = 16 * g + kb, e = k / (2 * tp), within = k % (2 * tp);
                    for (int p = 0; p < planes_in; ++p) bop[p][l][kb] = e < nelem ? (int8_t) staged(p, e, n - tp + 1 + within / 2, within & 1) : (int8_t) 0;
                }
            }
            // D = A B per pair of planes, into the lanes' registers
            int32_t d[2][2][64][4];                                    // [plane of A][plane of B][lane][register]
            for (int pa = 0; pa < 2; ++pa)
                for (int pb = 0; pb < planes_in; ++pb)
                    for (int i = 0; i < kBeamsRows; ++i)
                        for (int c = 0; c < kBeamsCols; ++c) {
                            int64_t s = 0;
                            for (int q = 0; q < 4; ++q)
                                for (int b = 0; b < 16; ++b) s += (int32_t) pl[pa * kBeamsPlaneBytes + (i + 16 * q) * 16 + b] * (int32_t) bop[pb][c + 16 * q][b];
                            if (std::llabs((long long) s) > ((int64_t) 1 << 20)) { std::fprintf(stderr, "a plane product leaves 2^20\n"); return 1; }
                            if (std::llabs((long long) s) > peak) peak = std::llabs((long long) s);
                            d[pa][pb][c + 16 * (i >> 2)][i & 3] = (int32_t) s;
                        }
            for (int l = 0; l < 64; ++l) {
                const int col = l & 15, g = l >> 4;
                const int64_t n = (int64_t) wave * TILE + (int64_t) S * col + j;
                if (n >= nsamp) continue;
                for (int r = 0; r < 4; ++r) {
                    uint32_t acc;
                    if (in_size == 1) acc = (uint32_t) d[0][0][l][r] + ((uint32_t) d[1][0][l][r] << 8);
                    else acc = (uint32_t) d[0][0][l][r] + (((uint32_t) d[0][1][l][r] + (uint32_t) d[1][0][l][r]) << 8) + ((uint32_t) d[1][1][l][r] << 16) + (uint32_t) consts[4 * g + r];
                    const int b = 2 * g + (r >> 1), comp = r & 1;
                    int64_t want = 0;
                    if (b < nbeams)
                        for (int e = 0; e < nelem; ++e)
                            for (int t = 0; t < ntaps; ++t) {
                                const int64_t re = w[2 * (((size_t) b * nelem + e) * ntaps + t)], im = w[2 * (((size_t) b * nelem + e) * ntaps + t) + 1];
                                const int64_t xi = sc.at(e, n - t, 0), xq = sc.at(e, n - t, 1);
                                want += comp ? re * xq + im * xi : re * xi - im * xq;
                            }
                    if (std::llabs((long long) want) > peak_acc) peak_acc = std::llabs((long long) want);
                    if ((int64_t) (int32_t) acc != want) {
                        std::fprintf(stderr, "beam %d component %d sample %lld: the tile gives %d, the direct sum %lld\n", b, comp, (long long) n, (int32_t) acc, (long long) want);
                        return 1;
                    }
                }
            }
        }
    return std::printf("tile ok peak=%" PRId64 " acc=%" PRId64 "\n", peak, peak_acc) < 0;
}

int main()
{
    char what[16];
    long long a[9];
    const auto read = [&](int n) { for (int i = 0; i < n; ++i) if (std::scanf("%lld", &a[i]) != 1) return false; return true; };
    const auto shape_ok = [&]() { return a[0] >= 1 && a[0] <= kStapMaxElem && a[1] >= 1 && a[1] <= kStapMaxTaps && a[0] * a[1] <= kStapMaxRows && a[2] >= 1 && a[2] <= kBeamsMax; };
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "plan")) {
            if (!read(8)) return 2;
            if (!shape_ok() || a[3] < 0 || a[3] > INT32_MAX || (a[4] != 1 && a[4] != 2) || (a[5] != 1 && a[5] != 2) || a[6] < -32768 || a[6] > 32768) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (show_plan(plan_stap_beams((int) a[0], (int) a[1], (int) a[2], (int) a[3], (int) a[4], (int) a[5], (int) a[6], (int) a[7]), (int) a[0], (int) a[1], (int) a[3], (int) a[5], (int) a[6])) return 1;
        } else if (!std::strcmp(what, "split")) {
            if (!read(2)) return 2;
            if (a[0] < -32768 || a[1] > 32767) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (int rc = split((int) a[0], (int) a[1])) return rc;
        } else if (!std::strcmp(what, "planes")) {
            if (!read(5)) return 2;
            if (!shape_ok()) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (int rc = planes((int) a[0], (int) a[1], (int) a[2], (uint64_t) a[3], (int) a[4])) return rc;
        } else if (!std::strcmp(what, "tile")) {
            if (!read(9)) return 2;
            if (!shape_ok() || (a[3] != 1 && a[3] != 2) || (a[4] != 1 && a[4] != 2) || a[5] < 1 || a[7] < 0 || a[7] > 2 || a[8] < 0 || a[8] > 2) { std::fprintf(stderr, "request outside the ranges\n"); return 2; }
            if (int rc = tile((int) a[0], (int) a[1], (int) a[2], (int) a[3], (int) a[4], (int) a[5], (uint64_t) a[6], (int) a[7], (int) a[8])) return rc;
        } else if (!std::strcmp(what, "minrows")) {
            if (!read(2)) return 2;
            std::printf("rows=%d\n", beams_mfma_min_rows((int) a[0], (int) a[1]));
        } else if (!std::strcmp(what, "limits")) {
            std::printf("max_beams=%d max_entry=%d chunk8=%d chunk16=%d tile8=%d tile16=%d max_grid=%u gen_grid=%u threads=%d never=%d coef_dwords=%d\n", kBeamsMax,
                        kBeamsMaxEntry, beams_chunk_samples(1), beams_chunk_samples(2), beams_tile_samples(1), beams_tile_samples(2), kBeamsMaxGrid, kBeamsGenMaxGrid,
                        kBeamsThreads, kBeamsNever, kBeamsCoefDwords);
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
