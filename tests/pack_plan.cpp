// pack_plan.cpp -- csrc/gpsiq_pack_plan.h, the header gpsiq_pack / gpsiq_unpack / gpsiq_generate_batch_packed plan with, as a
// stand-alone program.  tests/test_pack_ref.py compiles and asks it, and also runs it built with -fsanitize=address,undefined.
// TEST INFRASTRUCTURE.  One request per line of stdin:
//   pack   NBLOCKS NSAMP SAMPLE_SIZE BITS      -> "nothing" | "grid=.. threads=.. units=.. tiles=.. total=.. unit_src=.. unit_dst=.."
//   unpack NBLOCKS NSAMP BITS SAMPLE_SIZE      -> the same; unit_src / unit_dst: bytes a unit reads / writes
//   piece  NBLOCKS SRC_BLOCK_BYTES OVERRIDE    -> "piece=.."
//   bytes  NSAMP BITS                          -> "bytes=.."
// Every answer is first held to what a plan must hold whatever was asked: the units cover the block's wide side exactly once (the
// last one may be ragged), the tiles cover the units, the grid is non-empty and within its limit.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "gpsiq_pack_plan.h"

static int show(const gpsiq::PackPlan &p, int nblocks, uint64_t side, int unit_wide, int unit_src, int unit_dst)
{
    if (!p.launch) return std::printf("nothing\n") < 0;
    const uint64_t per_tile = (uint64_t) gpsiq::kPackThreads * gpsiq::kPackUnitsPerThread;
    if ((uint64_t) p.units * unit_wide < side || (uint64_t) (p.units - 1) * unit_wide >= side || (uint64_t) p.tiles * per_tile < p.units ||
        (uint64_t) (p.tiles - 1) * per_tile >= p.units || p.total != (uint64_t) p.tiles * (uint64_t) nblocks || p.grid < 1 ||
        p.grid > gpsiq::kPackMaxGrid || (uint64_t) p.grid > p.total || (p.total <= gpsiq::kPackMaxGrid && p.grid != p.total) ||
        p.threads != (unsigned) gpsiq::kPackThreads) {
        std::fprintf(stderr, "plan does not hold its own invariants\n");
        return 1;
    }
    return std::printf("grid=%u threads=%u units=%" PRIu32 " tiles=%" PRIu32 " total=%" PRIu64 " unit_src=%d unit_dst=%d\n", p.grid, p.threads, p.units,
                       p.tiles, p.total, unit_src, unit_dst) < 0;
}

int main()
{
    char what[16];
    long long a, b, c, d;
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "pack") || !std::strcmp(what, "unpack")) {
            if (std::scanf("%lld %lld %lld %lld", &a, &b, &c, &d) != 4) return 2;
            const bool pk = what[0] == 'p';
            const int ss = (int) (pk ? c : d), bits = (int) (pk ? d : c);
            const gpsiq::PackPlan p = pk ? gpsiq::plan_pack((int) a, (int) b, ss, bits) : gpsiq::plan_unpack((int) a, (int) b, bits, ss);
            const uint64_t side = b > 0 ? (uint64_t) 2 * (uint64_t) b * (uint64_t) ss : 0;
            const bool ok = gpsiq::pack_format_ok(ss, bits);
            const int us = !ok ? 0 : pk ? gpsiq::pack_unit_src_bytes(ss, bits) : gpsiq::unpack_unit_src_bytes();
            const int ud = !ok ? 0 : pk ? gpsiq::pack_unit_dst_bytes(ss, bits) : gpsiq::unpack_unit_dst_bytes(bits, ss);
            if (show(p, (int) a, side, pk ? us : ud, us, ud)) return 1;
        } else if (!std::strcmp(what, "piece")) {
            if (std::scanf("%lld %lld %lld", &a, &b, &c) != 3) return 2;
            const int n = gpsiq::pack_piece_blocks((int) a, (size_t) b, (long) c);
            if (a > 0 && (n < 1 || n > a)) { std::fprintf(stderr, "piece outside [1, nblocks]\n"); return 1; }
            std::printf("piece=%d\n", n);
        } else if (!std::strcmp(what, "bytes")) {
            if (std::scanf("%lld %lld", &a, &b) != 2) return 2;
            std::printf("bytes=%zu\n", gpsiq::packed_block_bytes((int) a, (int) b));
        } else {
            std::fprintf(stderr, "unknown request %s\n", what);
            return 2;
        }
    }
    return 0;
}
