// follow_plan.cpp -- plan_follow() of csrc/gpsiq_follow_plan.h, the header gpsiq_follow itself plans with, as a stand-alone program: the
// grid, the epochs per launch and the launches a call takes.  tests/_follow_plan.py compiles and asks it; tests/test_follow_ref.py also
// runs it built with -fsanitize=address,undefined.  Host code only.  TEST INFRASTRUCTURE.
//   follow_plan NSAMP SAMPLE_SIZE NPRN MAX_EPOCHS KNOB RECORDS     one request (KNOB: the value of GPSIQ_FOLLOW_EPOCHS_PER_LAUNCH, 0 for none;
//                                                                  RECORDS: the most records any satellite of the call ended with)
//   follow_plan -                                                  the same, one request per line of stdin
// answer: "nothing", or "grid=.. threads=.. per_launch=.. records=.. record_bytes=.. max_launches=.. launches=.."
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gpsiq_follow_plan.h"

static int answer(long long nsamp, int ss, int nprn, long long max_epochs, long long knob, long long records)
{
    using namespace gpsiq;
    const FollowPlan p = plan_follow(nsamp, ss, nprn, max_epochs, knob);
    if (p.kind != kPlanLaunch) return std::printf("nothing\n") < 0;
    const int launches = follow_launches(records, p.epochs_per_launch);
    // what every plan must hold, whatever was asked
    const bool ok = p.grid == (unsigned) nprn && p.grid <= (unsigned) kFollowMaxPrn && p.threads == (unsigned) kFollowThreads && p.threads % 64 == 0 &&
                    p.epochs_per_launch >= 1 && p.epochs_per_launch <= kFollowEpochsPerLaunch && p.records == (uint64_t) nprn * (uint64_t) max_epochs &&
                    p.record_bytes == p.records * kFollowRecordBytes && p.record_bytes <= kFollowRecordCap && p.max_launches >= 1 &&
                    (records > max_epochs || records > nsamp || launches <= p.max_launches) &&
                    (int64_t) (p.max_launches - 1) * p.epochs_per_launch <= (max_epochs < nsamp ? max_epochs : nsamp);
    if (!ok) {
        std::fprintf(stderr, "plan does not hold its own invariants\n");
        return 1;
    }
    return std::printf("grid=%u threads=%u per_launch=%d records=%" PRIu64 " record_bytes=%" PRIu64 " max_launches=%d launches=%d\n", p.grid, p.threads,
                       p.epochs_per_launch, p.records, p.record_bytes, p.max_launches, launches) < 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "-")) {
        long long nsamp, max_epochs, knob, records;
        int ss, nprn;
        while (std::scanf("%lld %d %d %lld %lld %lld", &nsamp, &ss, &nprn, &max_epochs, &knob, &records) == 6)
            if (answer(nsamp, ss, nprn, max_epochs, knob, records)) return 1;
        return 0;
    }
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s NSAMP SAMPLE_SIZE NPRN MAX_EPOCHS KNOB RECORDS   or   %s -\n", argv[0], argv[0]);
        return 2;
    }
    return answer(std::atoll(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]), std::atoll(argv[6]));
}
