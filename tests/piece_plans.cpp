// piece_plans.cpp -- the piece plans of the batch calls (csrc/gpsiq_pieces.h), printed for a grid of rates, channel counts, block
// counts and GPSIQ_PIECE_BLOCKS overrides.  TEST INFRASTRUCTURE: tests/test_piece_plans.py holds the lines against its tables.
//   one line per planner and configuration; on it the result without the override, then with it at 0 1 2 3 5 8 40 -1 (" | ")
//   a list of pieces is printed as their sizes, runs of equal sizes as size x count
// With the argument "handover": the phase hand-over between the pieces of the staged batch calls (piece_rows), one line per case.
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "gpsiq_pieces.h"

using namespace gpsiq;

static const std::optional<long> kOverrides[] = {std::nullopt, 0, 1, 2, 3, 5, 8, 40, -1};
static const int kNsamp[] = {260000, 1000000, 2500000};            // 0.1 s blocks at 2.6, 10 and 25 Msps
static const double kRates[] = {6.0e12, 1.5e12};                    // channel-samples/s: the default, and one that makes 25 Msps kernel-bound

static std::string sizes(const std::vector<int> &ends, int first = 0)
{
    std::string s;
    int prev = first;
    for (size_t k = 0; k < ends.size();) {
        const int size = ends[k] - prev;
        size_t run = 1;
        while (k + run < ends.size() && ends[k + run] - ends[k + run - 1] == size) ++run;
        s += (s.empty() ? "" : " ") + std::to_string(size) + (run > 1 ? "x" + std::to_string(run) : "");
        prev = ends[k + run - 1];
        k += run;
    }
    return s;
}

template <class F> static void line(const std::string &head, F result)
{
    std::string s = head + ":";
    for (size_t k = 0; k < sizeof kOverrides / sizeof kOverrides[0]; ++k) s += (k ? " | " : " ") + result(kOverrides[k]);
    std::printf("%s\n", s.c_str());
}

// Five blocks of nchan slots cut at block 2.  Slot i is of kind (i + shift) % 4: 0 keeps its satellite across the edge, 1 changes it
// there, 2 has none (prn 0) on either side, 3 loses it there (prn 0 from the edge on).  Every carr_phase and every carried phase is a
// value of its own, so a row that took the wrong one shows.  Returns the number of checks that failed.
static int handover_case(int nchan, int shift)
{
    const int nblocks = 5, b0 = 2, nb = nblocks - b0;
    std::vector<gpsiq_chan_t> ch((size_t) nblocks * nchan);
    std::memset(ch.data(), 0, ch.size() * sizeof(gpsiq_chan_t));
    double carr[GPSIQ_MAX_CHAN];
    for (int i = 0; i < GPSIQ_MAX_CHAN; ++i) carr[i] = -7.5 - i;
    for (int b = 0; b < nblocks; ++b)
        for (int i = 0; i < nchan; ++i) {
            gpsiq_chan_t &r = ch[(size_t) b * nchan + i];
            const int kind = (i + shift) % 4;
            r.prn = kind == 0 ? i + 1 : kind == 1 ? (b < b0 ? i + 1 : i + 17) : kind == 2 ? 0 : (b < b0 ? i + 1 : 0);
            r.carr_phase = 1000.0 * b + i + 0.25;
            r.f_carr = 10.0 * b + i;
        }
    const std::vector<gpsiq_chan_t> before = ch;
    int bad = 0;
    std::vector<gpsiq_chan_t> row;
    // piece 0: the caller's rows as they lie, nothing copied
    bad += piece_rows(ch.data(), 0, b0, nchan, carr, &row) != ch.data() || !row.empty();
    // a later piece: a copy, its first row rewritten where the slot keeps its satellite, every other byte the caller's
    const gpsiq_chan_t *rows = piece_rows(ch.data(), b0, nb, nchan, carr, &row);
    bad += rows != row.data() || row.size() != (size_t) nb * nchan || rows == ch.data() + (size_t) b0 * nchan;
    for (int i = 0; i < nchan; ++i) {
        const int kind = (i + shift) % 4;
        gpsiq_chan_t want = before[(size_t) b0 * nchan + i];
        if (kind == 0) want.carr_phase = carr[i];                     // kinds 1, 2, 3: its own carr_phase, untouched
        bad += std::memcmp(&rows[i], &want, sizeof want) != 0;
        bad += kind == 0 && rows[i].carr_phase == before[(size_t) b0 * nchan + i].carr_phase;
    }
    bad += std::memcmp(rows + nchan, before.data() + (size_t) (b0 + 1) * nchan, (size_t) (nb - 1) * nchan * sizeof(gpsiq_chan_t)) != 0;
    bad += std::memcmp(ch.data(), before.data(), ch.size() * sizeof(gpsiq_chan_t)) != 0;      // the caller's rows are read only
    return bad;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "handover")) {
        int bad = 0;
        for (int nchan : {1, 3, GPSIQ_MAX_CHAN})
            for (int shift = 0; shift < 4; ++shift) {
                const int b = handover_case(nchan, shift);
                std::printf("handover nchan=%d shift=%d: %s\n", nchan, shift, b ? "WRONG" : "ok");
                bad += b;
            }
        return bad != 0;
    }
    for (int nsamp : {260000, 1000000, 2500000, 33333})
        for (int ss : {1, 2}) {
            const size_t stride = ((size_t) 2 * nsamp * ss + 15) & ~(size_t) 15;
            line("d2h nsamp=" + std::to_string(nsamp) + " ss=" + std::to_string(ss),
                 [&](std::optional<long> ov) { return std::to_string(d2h_chunk_blocks(stride, ov)); });
        }
    for (int nsamp : kNsamp)
        for (int nchan : {12, 16})
            for (double rate : kRates)
                for (int threads : {16, 4})
                    std::printf("kernel_bound nsamp=%d nchan=%d rate=%g threads=%d: %d\n", nsamp, nchan, rate, threads,
                                (int) ref_kernel_bound(nsamp, nchan, rate, threads));
    // fixed model, long batch into device memory: the nominal piece, and the pieces (the first an eighth of it, growing)
    for (int nsamp : kNsamp)
        for (int nblocks : {1, 100, 211, 212, 531, 532, 2047, 2048, 4000})
            line("fixed nsamp=" + std::to_string(nsamp) + " nblocks=" + std::to_string(nblocks), [&](std::optional<long> ov) {
                const int piece = batch_piece_blocks(nblocks, nsamp, ov);
                if (piece >= nblocks) return std::to_string(piece) + " one";
                std::vector<int> ends;
                piece_ends(0, nblocks, piece / 8 > 0 ? piece / 8 : 1, &ends, true);
                return std::to_string(piece) + " " + sizes(ends);
            });
    // reference model, host walk: chunk, kernel-bound or not (16 host threads), the head of a chain on the device, the pieces
    for (int nsamp : kNsamp)
        for (int nchan : {12, 16})
            for (double rate : kRates) {
                const int c4 = 4 * ref_chunk_blocks(1 << 30, nsamp, std::nullopt);
                for (int nblocks : {1, 40, c4, c4 + 1, 1200, 3000}) {
                    char head[128];
                    std::snprintf(head, sizeof head, "reference nsamp=%d nchan=%d rate=%g nblocks=%d", nsamp, nchan, rate, nblocks);
                    line(head, [&](std::optional<long> ov) {
                        const int chunk = ref_chunk_blocks(nblocks, nsamp, ov);
                        const bool kb = ref_kernel_bound(nsamp, nchan, rate, 16);
                        std::vector<int> ends;
                        piece_ends(0, nblocks, chunk, &ends, kb);
                        return std::to_string(chunk) + (kb ? " kb" : "") + " head=" + std::to_string(ref_head(ends, nblocks, nsamp, nchan, rate)) +
                               " " + sizes(ends);
                    });
                }
            }
    // two devices' ranges of one timeline (gpsiq_generate_batch_multi): pieces never straddle them
    for (int nsamp : kNsamp)
        line("reference ranges nsamp=" + std::to_string(nsamp) + " 0-700 700-1400", [&](std::optional<long> ov) {
            std::vector<int> ends;
            for (int r0 : {0, 700}) piece_ends(r0, 700, ref_chunk_blocks(700, nsamp, ov), &ends, false);
            return sizes(ends);
        });
    // device evaluation: descriptors in host memory or on the device, either NCO model
    for (int nsamp : kNsamp)
        for (int nchan : {12, 16})
            for (int host_rows : {0, 1})
                for (int reference : {0, 1})
                    for (int nblocks : {1, 31, 32, 33, 200, 1100, 30000, 1000000}) {
                        char head[128];
                        std::snprintf(head, sizeof head, "device nsamp=%d nchan=%d host_rows=%d reference=%d nblocks=%d", nsamp, nchan, host_rows,
                                      reference, nblocks);
                        line(head, [&](std::optional<long> ov) {
                            std::vector<int> ends;
                            device_piece_ends(nblocks, nsamp, nchan, host_rows, reference, 6.0e12, ov, 8, &ends);
                            return sizes(ends);
                        });
                    }
    return 0;
}
