// launch_plans.cpp -- the launch plans of the synthesis kernels (csrc/gpsiq_launch_plan.h), printed for a grid of variants, sample
// formats, block lengths and counts, channel counts, amplitude bounds, noise / level states and grid-shape policies.
// TEST INFRASTRUCTURE: tests/test_launch_plans.py holds the lines against its table.
//   one line per run of equal plans along the field that is swept (the last one before "->"); a plan is printed as the launches
//   it stands for: kernel<template arguments> grid= block= args= (nsamp and the kernel's shape arguments), "none" where there is
//   nothing to render, "invalid" where the variant has no noise / level path
#include <cstdio>
#include <string>

#include "gpsiq_launch_plan.h"

using namespace gpsiq;

// one launch request; the defaults are the flagship shape (2.6 Msps blocks, int16, eight channels, nothing switched on)
struct In {
    int  v = 5, ss = 2, n = 260000, nb = 200, act = 8;
    long amp = 1000, z = 0;         // z: max |noise| while the noise is on, 0 = off
    int  lv = 0, scr = 1, fast = 1, pol = 0;
};

static std::string plan_string(const In &in)
{
    SegPolicy pol;
    if (in.pol) { pol.tail_wgs = 64; pol.max_wave_rows = 128; pol.setup_rows = 10.0; pol.drain_rounds = 2.0; }
    pol.allow_fast = in.fast != 0;
    SynthClass cls;
    cls.max_active = in.act;
    cls.max_amplitude = in.amp;
    const SynthPlan p = plan_synth(in.v, in.n, in.nb, in.ss, cls, in.scr != 0, {in.z != 0 || in.lv != 0, in.z, in.lv != 0}, pol);
    if (p.kind == kPlanNothing) return "none";
    if (p.kind == kPlanNoPath) return "invalid";
    auto num = [](long v) { return std::to_string(v); };
    const std::string n = num(in.n), fmt = num(in.ss), shape = " grid=" + num(p.grid) + " block=" + num(p.threads) + " args=" + n + ",";
    switch (p.variant) {
    case kGeneric: return "synth_generic<" + fmt + ">" + shape + num(p.tiles) + "," + num(p.tile_samples);
    case kRows:    return "synth_rows<" + fmt + ">" + shape + num(p.tiles);
    case kRowsX:   return "synth_rowsx<" + fmt + ", " + num(p.slots) + ">" + shape + num(p.tiles);
    case kSegMask:
        return "sign_masks grid=" + num(p.pre_grid) + " block=" + num(kMaskThreads) + " args=" + n + "," + num(in.nb) + "," + num(p.rows_total) + "," +
               num(p.rowgroups) + " ; synth_mask<" + fmt + ", " + num(p.slots) + ">" + shape + num(p.rows_total) + "," + num(p.tiles) + "," + num(p.wave_rows);
    default: break;
    }
    const char *family[] = {"synth_tile", "synth_tile_noise", "synth_tile_level"};
    return std::string(family[p.family]) + "<" + fmt + ", " + num(p.slots) + ", " + num(p.rows) + ", " + num(p.H) + ", " + (p.fast ? "true" : "false") +
           (p.variant == kSegBoth ? ", " + num(kWaves) + ", true>" : ">") + shape + num(p.tiles) + "," + num(p.wave_rows) + "," + num(p.big_wgs) + "," +
           num(p.big_blocks) + "," + num(p.tiles_small);
}

// ---- the grid ---------------------------------------------------------------------------------------------------------------

static const int kNsamp[] = {0, 1, 63, 64, 65, 16383, 16384, 16385, 33333, 102300, 260000, 1000000, 2500000};
static const int kNblocks[] = {1, 2, 3, 7, 26, 200, 2000, 4130};
static const int kActive[] = {1, 4, 5, 8, 9, 12, 13, 16};
static const long kAmp[] = {0, 32667, 32767, 32768};

// the request without the field that a sweep varies
static std::string head(const In &in, const char *skip)
{
    std::string s = variant_name(in.v);
    auto put = [&](const char *key, long val) { if (std::string(key) != skip) s += std::string(" ") + key + "=" + std::to_string(val); };
    put("ss", in.ss); put("n", in.n); put("nb", in.nb); put("act", in.act); put("amp", in.amp); put("z", in.z);
    put("lv", in.lv); put("scr", in.scr); put("fast", in.fast); put("pol", in.pol);
    return s;
}

// one line per run of equal plans along the swept field
static std::string g_head, g_key, g_vals, g_plan;
static void flush()
{
    if (!g_head.empty()) std::printf("%s %s=%s -> %s\n", g_head.c_str(), g_key.c_str(), g_vals.c_str(), g_plan.c_str());
    g_head.clear();
}
static void point(const In &in, const char *key, long val)
{
    const std::string h = head(in, key), p = plan_string(in);
    if (h == g_head && key == g_key && p == g_plan) { g_vals += "," + std::to_string(val); return; }
    flush();
    g_head = h; g_key = key; g_vals = std::to_string(val); g_plan = p;
}

static void grid()
{
    // block lengths either side of a row, a one-chunk workgroup, a generic tile, max_wave_rows
    for (int v = 0; v < 9; ++v)
        for (int n : kNsamp) { In in; in.v = v; in.n = n; point(in, "n", n); }
    // block counts: no tail, a tail capped at half the blocks, the whole tail
    for (int v = 0; v < 9; ++v)
        for (int n : {260000, 2500000})
            for (int nb : kNblocks) {
                if (v < 4 && (n != 260000 || (nb != 1 && nb != 4130))) continue;      // their grid is tiles x blocks
                In in; in.v = v; in.n = n; in.nb = nb; point(in, "nb", nb);
            }
    { In in; in.nb = 0; point(in, "nb", 0); }
    // int8 output
    for (int v = 0; v < 9; ++v)
        for (int n : {65, 260000}) { In in; in.v = v; in.ss = 1; in.n = n; point(in, "n", n); }
    // channel slots
    for (int v = 3; v < 9; ++v)
        for (int ss : {2, 1})
            for (int act : kActive) { In in; in.v = v; in.ss = ss; in.act = act; point(in, "act", act); }
    // the plain-add rule and the fall-backs: amplitude bound x noise x level x GPSIQ_NO_FAST (x scratch for segm)
    for (int v = 4; v <= 6; ++v)
        for (int ss : {2, 1})
            for (long z : {0L, 100L, 40000L})
                for (int lv : {0, 1})
                    for (int fast : {1, 0})
                        for (long amp : kAmp) { In in; in.v = v; in.ss = ss; in.z = z; in.lv = lv; in.fast = fast; in.amp = amp; point(in, "amp", amp); }
    for (int ss : {2, 1})
        for (int scr : {1, 0})
            for (int fast : {1, 0})
                for (long amp : kAmp) { In in; in.v = 7; in.ss = ss; in.scr = scr; in.fast = fast; in.amp = amp; point(in, "amp", amp); }
    for (int ss : {2, 1})
        for (int fast : {1, 0})
            for (long amp : kAmp) { In in; in.v = 8; in.ss = ss; in.fast = fast; in.amp = amp; point(in, "amp", amp); }
    // noise and level on the variants without such a path (and generic, which has one)
    for (int v : {0, 1, 2, 3, 7, 8})
        for (int lv : {0, 1})
            for (long z : {0L, 100L}) { In in; in.v = v; in.lv = lv; in.z = z; if (lv || z) point(in, "z", z); }
    // another grid-shape policy
    for (int v : {4, 5, 6, 8})
        for (int n : {65, 16385, 260000, 2500000})
            for (int nb : {7, 200})
                for (int pol : {0, 1}) { In in; in.v = v; in.n = n; in.nb = nb; in.pol = pol; point(in, "pol", pol); }
    flush();
}

int main()
{
    grid();
    // the automatic choice at its two thresholds, and segm's scratch
    for (uint64_t edge : {kRowsMaxCodeStep, kHalfRowsMaxCodeStep})
        for (int d = -1; d <= 1; ++d)
            std::printf("auto_variant %s%+d -> %s\n", edge == kRowsMaxCodeStep ? "kRowsMaxCodeStep" : "kHalfRowsMaxCodeStep", d, variant_name(auto_variant(edge + d)));
    std::printf("auto_variant 0 -> %s\n", variant_name(auto_variant(0)));
    for (int v = 0; v < kNumVariants; ++v)
        std::printf("scratch %s -> %zu %zu %zu %zu %zu\n", variant_name(v), variant_scratch_bytes(v, 260000, 200), variant_scratch_bytes(v, 64, 1),
                    variant_scratch_bytes(v, 65, 3), variant_scratch_bytes(v, 0, 3), variant_scratch_bytes(v, 65, 0));
    return 0;
}
