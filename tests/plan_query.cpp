// plan_query.cpp -- the kernel plan_synth() (csrc/gpsiq_launch_plan.h) yields for ONE launch request, in the kernel spelling of
// tests/launch_plans.cpp.  TEST INFRASTRUCTURE: tests/_plan_query.py compiles and asks it, so that a GPU test can assert which
// instantiation a launch takes before it compares the bytes, and tests/test_stage_cases.py can hold the case table of the stage
// kernels against the list of kernels that exist.
//   plan_query VARIANT SS NSAMP NBLOCKS ACTIVE AMP MAXZ LEVEL FAST TAIL_WGS MAX_WAVE_ROWS SETUP_ROWS DRAIN
//     VARIANT  generic | tile | seg | segh | ... (variant_name) or its number; never auto: the caller resolves it as the library does
//     MAXZ     max |z| of the noise table, -1 = the noise is off
//     LEVEL    1 = the output level stage is on
//     FAST     SegPolicy::allow_fast (0 under GPSIQ_NO_FAST=1)
//     the four grid-shape numbers of SegPolicy; "-" keeps the header's default
//   plan_query -          the same thirteen fields per line of standard input, one answer per line
//   answer: "<kernel> ; stage=<plain|noise|level> variant=<name> rows= wave_rows= tiles= big_wgs= big_blocks= tiles_small= grid=",
//   or "none" / "invalid" as launch_plans.cpp prints them
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "gpsiq_launch_plan.h"

using namespace gpsiq;

static bool variant_of(const std::string &s, int *v)
{
    for (int i = 0; i < kNumVariants; ++i)
        if (s == variant_name(i)) { *v = i; return true; }
    char *end = nullptr;
    const long n = std::strtol(s.c_str(), &end, 10);
    if (end == s.c_str() || *end || n < 0 || n >= kNumVariants) return false;
    *v = (int) n;
    return true;
}

static bool answer(const std::vector<std::string> &f, std::string *out)
{
    if (f.size() != 13) return false;
    int v = 0;
    if (!variant_of(f[0], &v) || v == kAuto) return false;
    const int ss = std::atoi(f[1].c_str()), n = std::atoi(f[2].c_str()), nb = std::atoi(f[3].c_str());
    SynthClass cls;
    cls.max_active = std::atoi(f[4].c_str());
    cls.max_amplitude = std::atol(f[5].c_str());
    const long z = std::atol(f[6].c_str());
    const bool level = std::atoi(f[7].c_str()) != 0;
    SegPolicy pol;
    pol.allow_fast = std::atoi(f[8].c_str()) != 0;
    if (f[9] != "-") pol.tail_wgs = std::atoi(f[9].c_str());
    if (f[10] != "-") pol.max_wave_rows = std::atoi(f[10].c_str());
    if (f[11] != "-") pol.setup_rows = std::atof(f[11].c_str());
    if (f[12] != "-") pol.drain_rounds = std::atof(f[12].c_str());
    const SynthPlan p = plan_synth(v, n, nb, ss, cls, true, {z >= 0 || level, z >= 0 ? z : 0, level}, pol);
    if (p.kind == kPlanNothing) { *out = "none"; return true; }
    if (p.kind == kPlanNoPath) { *out = "invalid"; return true; }
    auto num = [](long x) { return std::to_string(x); };
    const std::string fmt = num(ss);
    std::string k;
    switch (p.variant) {
    case kGeneric: k = "synth_generic<" + fmt + ">"; break;
    case kRows:    k = "synth_rows<" + fmt + ">"; break;
    case kRowsX:   k = "synth_rowsx<" + fmt + ", " + num(p.slots) + ">"; break;
    case kSegMask: k = "synth_mask<" + fmt + ", " + num(p.slots) + ">"; break;
    default: {
        const char *family[] = {"synth_tile", "synth_tile_noise", "synth_tile_level"};
        k = std::string(family[p.family]) + "<" + fmt + ", " + num(p.slots) + ", " + num(p.rows) + ", " + num(p.H) + ", " + (p.fast ? "true" : "false") +
            (p.variant == kSegBoth ? ", " + num(kWaves) + ", true>" : ">");
    }
    }
    const char *stage[] = {"plain", "noise", "level"};
    *out = k + " ; stage=" + stage[p.family] + " variant=" + variant_name(p.variant) + " rows=" + num(p.rows) + " wave_rows=" + num(p.wave_rows) +
           " tiles=" + num(p.tiles) + " big_wgs=" + num(p.big_wgs) + " big_blocks=" + num(p.big_blocks) + " tiles_small=" + num(p.tiles_small) +
           " grid=" + num(p.grid);
    return true;
}

int main(int argc, char **argv)
{
    std::string out;
    if (argc == 2 && std::strcmp(argv[1], "-") == 0) {
        char line[512];
        while (std::fgets(line, sizeof line, stdin)) {
            std::istringstream is(line);
            std::vector<std::string> f;
            for (std::string w; is >> w;) f.push_back(w);
            if (f.empty()) continue;
            if (!answer(f, &out)) { std::fprintf(stderr, "plan_query: bad request: %s", line); return 2; }
            std::printf("%s\n", out.c_str());
        }
        return 0;
    }
    if (!answer(std::vector<std::string>(argv + 1, argv + argc), &out)) {
        std::fprintf(stderr, "usage: plan_query VARIANT SS NSAMP NBLOCKS ACTIVE AMP MAXZ LEVEL FAST TAIL_WGS MAX_WAVE_ROWS SETUP_ROWS DRAIN | plan_query -\n");
        return 2;
    }
    std::printf("%s\n", out.c_str());
    return 0;
}
