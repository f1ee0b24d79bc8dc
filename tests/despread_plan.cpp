// despread_plan.cpp -- plan_despread() of csrc/gpsiq_despread_plan.h, the header gpsiq_despread itself plans with, as a stand-alone
// program: which correlator kernel and grid a call takes.  tests/_despread_plan.py compiles and asks it; tests/test_despread_ref.py
// also runs it built with -fsanitize=address,undefined.  TEST INFRASTRUCTURE.
//   despread_plan NSAMP NBLOCKS SEG_LEN MAX_CODE_STEP MAX_ACTIVE FORCE_GENERIC TARGET_WGS        one request ("-" as TARGET_WGS: default)
//   despread_plan -                                                                                the same, one request per line of stdin
// answer: "nothing", or "kernel=rows slots=16 grid=.. threads=.. tiles=.. wave_rows=.. seg_rows=.. nseg=.."
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gpsiq_despread_plan.h"

static int answer(int nsamp, int nblocks, int seg_len, uint64_t step, int active, int force, const char *target)
{
    gpsiq::SynthClass cls;
    cls.max_code_step = step;
    cls.max_active = active;
    const int t = std::strcmp(target, "-") ? std::atoi(target) : gpsiq::kDespreadTargetWgs;
    const gpsiq::DespreadPlan p = gpsiq::plan_despread(nsamp, nblocks, seg_len, cls, force != 0, t);
    if (p.kind != gpsiq::kPlanLaunch) return std::printf("nothing\n") < 0;
    // what every plan must hold, whatever was asked: the runs cover the block, a row lies in one segment, no wave is longer than
    // the partial sums allow between two widenings of a chunk
    const int rows_total = (int) (((int64_t) nsamp + 63) / 64);      // (no int overflow next to INT_MAX)
    if ((int64_t) p.tiles * gpsiq::kDespreadWaves * p.wave_rows < rows_total || p.seg_rows * 64 != seg_len ||
        (int64_t) p.nseg * seg_len < nsamp || p.grid != (unsigned) p.tiles * (unsigned) nblocks || p.wave_rows < 1 ||
        (p.kernel == gpsiq::kDespreadRows && (p.wave_rows % gpsiq::kDespreadChunkRows || p.wave_rows > gpsiq::kDespreadMaxWaveRows))) {
        std::fprintf(stderr, "plan does not hold its own invariants\n");
        return 1;
    }
    return std::printf("kernel=%s slots=%d grid=%u threads=%u tiles=%d wave_rows=%d seg_rows=%d nseg=%d\n", gpsiq::despread_kernel_name(p.kernel),
                       p.slots, p.grid, p.threads, p.tiles, p.wave_rows, p.seg_rows, p.nseg) < 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "-")) {
        int nsamp, nblocks, seg_len, active, force;
        uint64_t step;
        char target[32];
        while (std::scanf("%d %d %d %" SCNu64 " %d %d %31s", &nsamp, &nblocks, &seg_len, &step, &active, &force, target) == 7)
            if (answer(nsamp, nblocks, seg_len, step, active, force, target)) return 1;
        return 0;
    }
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s NSAMP NBLOCKS SEG_LEN MAX_CODE_STEP MAX_ACTIVE FORCE_GENERIC TARGET_WGS | -\n", argv[0]);
        return 2;
    }
    return answer(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::strtoull(argv[4], nullptr, 10), std::atoi(argv[5]),
                  std::atoi(argv[6]), argv[7]);
}
