// piece_plans.cpp -- the piece plans of the batch calls (csrc/gpsiq_pieces.h), printed for a grid of rates, channel counts, block
// counts and GPSIQ_PIECE_BLOCKS overrides.  TEST INFRASTRUCTURE: tests/test_piece_plans.py holds the lines against its tables.
//   one line per planner and configuration; on it the result without the override, then with it at 0 1 2 3 5 8 40 -1 (" | ")
//   a list of pieces is printed as their sizes, runs of equal sizes as size x count
#include <cstdio>
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

int main()
{
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
