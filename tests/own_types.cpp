// own_types.cpp -- the owning types the device context is made of and the one rule its groups of buffers grow by (csrc/gpsiq_own.h),
// and the first-use routines built from them: gpsiq_ctx::Chain::reserve, gpsiq_ctx::EvalDev::reserve / reserve_repair
// (csrc/gpsiq_ctx.h) and the reserve() of the four stream stages' sets (csrc/gpsiq_despread.h, gpsiq_pack.h, gpsiq_acquire.h,
// gpsiq_follow.h), on the CPU.
// TEST INFRASTRUCTURE: tests/test_own_types.py builds this file with the address and undefined-behaviour sanitizers and runs it.
// No HIP runtime is linked: the handful of entry points the two headers call are defined below as counting fakes over malloc /
// free.  Each fake counts its calls and the objects it has handed out that are still alive, aborts on a pointer it does not know
// (a double free), and can be told to fail its k-th call; the creating ones (allocations, events, streams) also share one
// sequence number, so that "the k-th resource a routine makes" can be made to fail whatever its kind.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>

#include "gpsiq_ctx.h"

namespace {

struct Fake { const char *name; long calls, fail_at, live; };      // fail_at: this call (counted from 1) fails; 0: none
Fake f_malloc = {"hipMalloc", 0, 0, 0}, f_free = {"hipFree", 0, 0, 0}, f_hmalloc = {"hipHostMalloc", 0, 0, 0}, f_hfree = {"hipHostFree", 0, 0, 0},
     f_ev = {"hipEventCreateWithFlags", 0, 0, 0}, f_evdel = {"hipEventDestroy", 0, 0, 0}, f_st = {"hipStreamCreate*", 0, 0, 0},
     f_stdel = {"hipStreamDestroy", 0, 0, 0};
Fake *const kFakes[] = {&f_malloc, &f_free, &f_hmalloc, &f_hfree, &f_ev, &f_evdel, &f_st, &f_stdel};
long g_created = 0, g_fail_created_at = 0;                         // across the creating fakes
size_t g_last_bytes = 0;
unsigned g_last_flags = 0;
int g_last_priority = 0;
std::set<void *> g_live[4];                                        // device, page-locked, events, streams

[[noreturn]] void die(const char *what, const char *name)
{
    std::fprintf(stderr, "own_types: %s (%s)\n", what, name);
    std::abort();
}
#define CHECK(cond) do { if (!(cond)) die("check failed: " #cond, __func__); } while (0)

bool fails(Fake &f, bool creates)
{
    ++f.calls;
    if (creates) ++g_created;
    return f.calls == f.fail_at || (creates && g_created == g_fail_created_at);
}
hipError_t make(Fake &f, int kind, void **out, size_t bytes)
{
    if (fails(f, true)) return hipErrorOutOfMemory;
    g_last_bytes = bytes;
    *out = std::malloc(bytes ? bytes : 1);
    g_live[kind].insert(*out);
    ++f.live;
    return hipSuccess;
}
// a release that fails gives nothing back: the object stays alive in the runtime, as it would in the real one
hipError_t drop(Fake &f, Fake &maker, int kind, void *p)
{
    if (!g_live[kind].count(p)) die("released twice, or never handed out", f.name);
    if (fails(f, false)) return hipErrorInvalidValue;
    g_live[kind].erase(p);
    std::free(p);
    --maker.live;
    return hipSuccess;
}
long live_total() { long n = 0; for (auto &s : g_live) n += (long) s.size(); return n; }
void reset()
{
    CHECK(live_total() == 0);                                      // (g) every scenario ends with nothing alive
    for (Fake *f : kFakes) { CHECK(f->live == 0); f->calls = 0; f->fail_at = 0; }
    g_created = 0; g_fail_created_at = 0;
}
long calls_total() { long n = 0; for (Fake *f : kFakes) n += f->calls; return n; }

}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return make(f_malloc, 0, p, bytes); }
hipError_t hipFree(void *p) { return drop(f_free, f_malloc, 0, p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags) { g_last_flags = flags; return make(f_hmalloc, 1, p, bytes); }
hipError_t hipHostFree(void *p) { return drop(f_hfree, f_hmalloc, 1, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { g_last_flags = flags; return make(f_ev, 2, reinterpret_cast<void **>(e), 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop(f_evdel, f_ev, 2, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) { g_last_flags = flags; g_last_priority = 0; return make(f_st, 3, reinterpret_cast<void **>(s), 1); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned flags, int priority)
{
    g_last_flags = flags; g_last_priority = priority;
    return make(f_st, 3, reinterpret_cast<void **>(s), 1);
}
hipError_t hipStreamDestroy(hipStream_t s) { return drop(f_stdel, f_st, 3, s); }
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) { *least = 1; *greatest = -2; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "fake error"; }
}

// what HIP_TRY reports through: the last text is kept, as the library does
static char g_error[400];
namespace gpsiq {
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}
}

using gpsiq::DevBuf;
using gpsiq::PinnedBuf;
using gpsiq::Event;
using gpsiq::Stream;
using gpsiq::DespreadSet;
using gpsiq::PackSet;
using gpsiq::PieceRing;
using gpsiq::AcquireSet;
using gpsiq::FollowSet;

// (a), (b): a buffer of either kind grows only, by one free and one allocation of exactly the count asked for
template <typename B>
static void grows_only(Fake &alloc, Fake &release)
{
    {
        B b;
        CHECK(b.get() == nullptr && b.cap() == 0);
        CHECK(b.reserve(0) == hipSuccess && calls_total() == 0);                 // nothing asked for, nothing done
        CHECK(b.reserve(10) == hipSuccess);
        CHECK(alloc.calls == 1 && release.calls == 0 && g_last_bytes == 10 * sizeof(*b.get()) && b.cap() == 10 && b.get());
        auto *first = b.get();
        for (size_t n : {(size_t) 10, (size_t) 9, (size_t) 1, (size_t) 0}) CHECK(b.reserve(n) == hipSuccess);
        CHECK(calls_total() == 1 && b.get() == first && b.cap() == 10);          // (a) at or below the capacity: no call at all
        CHECK(b.reserve(11) == hipSuccess);
        CHECK(alloc.calls == 2 && release.calls == 1 && calls_total() == 3);     // (b) one free, one allocation ...
        CHECK(g_last_bytes == 11 * sizeof(*b.get()) && b.cap() == 11);           // ... of exactly the count given
        CHECK(alloc.live == 1);
    }
    CHECK(release.calls == 2);                                                   // the destructor gives the last one back
    reset();
}

// (c): an allocation that fails leaves the buffer empty; the next reserve succeeds; nothing is freed twice
template <typename B>
static void survives_failed_allocation(Fake &alloc, Fake &release)
{
    {
        B b;
        alloc.fail_at = 1;
        CHECK(b.reserve(8) == hipErrorOutOfMemory && !b.get() && b.cap() == 0);  // the first allocation of all
        CHECK(b.reserve(8) == hipSuccess && b.cap() == 8);
        alloc.fail_at = 3;
        CHECK(b.reserve(100) == hipErrorOutOfMemory);                            // while growing: the old allocation is gone (freed once) ...
        CHECK(!b.get() && b.cap() == 0 && release.calls == 1 && alloc.live == 0);   // ... and the buffer does not claim it
        CHECK(b.reserve(4) == hipSuccess && b.cap() == 4 && release.calls == 1);    // starts over, with nothing to free
    }
    CHECK(release.calls == 2 && alloc.calls == 4);
    reset();
    { B b; alloc.fail_at = 1; CHECK(b.reserve(8) != hipSuccess); }               // destroyed empty: no release at all
    CHECK(release.calls == 0);
    reset();
}

// (d): a free that fails is reported, and the buffer has forgotten the pointer before: it is empty, and neither a later reserve
// nor the destructor hands the pointer to the runtime again (the fake would abort).  The runtime still holds that allocation.
template <typename B>
static void survives_failed_free(Fake &alloc, Fake &release, int kind)
{
    void *lost = nullptr;
    {
        B b;
        CHECK(b.reserve(8) == hipSuccess);
        lost = b.get();
        release.fail_at = 1;
        CHECK(b.reserve(16) == hipErrorInvalidValue);
        CHECK(!b.get() && b.cap() == 0 && alloc.calls == 1);                     // reported before anything new is allocated
        CHECK(b.reserve(16) == hipSuccess && b.cap() == 16 && b.get() != lost);
    }
    CHECK(release.calls == 2 && alloc.live == 1 && g_live[kind].count(lost));    // only the second allocation was ever released
    CHECK(drop(release, alloc, kind, lost) == hipSuccess);                       // (the test's own tidying up)
    reset();
}

// (e): ensure() makes the event / stream once, with the flags asked for
static void ensure_is_idempotent()
{
    {
        Event a, t;
        CHECK(!a.get());
        CHECK(a.ensure() == hipSuccess && g_last_flags == hipEventDisableTiming);
        hipEvent_t first = a.get();
        CHECK(first && a.ensure() == hipSuccess && a.ensure(hipEventDefault) == hipSuccess && a.get() == first && f_ev.calls == 1);
        CHECK(t.ensure(hipEventDefault) == hipSuccess && g_last_flags == hipEventDefault && f_ev.calls == 2);
        f_ev.fail_at = 3;
        Event b;
        CHECK(b.ensure() == hipErrorOutOfMemory && !b.get());
        CHECK(b.ensure() == hipSuccess && b.get());                              // a failed creation is tried again
        Stream s, p;
        CHECK(s.ensure() == hipSuccess && g_last_flags == hipStreamNonBlocking && g_last_priority == 0);
        hipStream_t sfirst = s.get();
        CHECK(s.ensure() == hipSuccess && s.ensure_greatest() == hipSuccess && s.get() == sfirst && f_st.calls == 1);
        CHECK(p.ensure_greatest() == hipSuccess && g_last_flags == hipStreamNonBlocking && g_last_priority == -2);   // the fake range's greatest
        CHECK(p.ensure_greatest() == hipSuccess && f_st.calls == 2);
        f_st.fail_at = 3;
        Stream q;
        CHECK(q.ensure() == hipErrorOutOfMemory && !q.get() && q.ensure() == hipSuccess && q.get());
    }
    CHECK(f_evdel.calls == 3 && f_stdel.calls == 3);
    reset();
}

// (f): a first-use set recovers from a failure at any of its resources.  `attempt` is the real routine on a fresh set; with
// the k-th resource it makes failing, the first attempt reports an error and the second completes the set: as many objects
// alive as after a clean first use, none made twice.  A third attempt makes no call.
template <typename Set, typename Attempt>
static void first_use_recovers(const char *what, Attempt attempt)
{
    long full = 0, made = 0;
    { Set s; CHECK(attempt(s) == GPSIQ_OK); full = live_total(); made = g_created; CHECK(full == made && full > 0); }
    reset();
    for (long k = 1; k <= made; ++k) {
        {
            Set s;
            g_fail_created_at = k;
            g_error[0] = 0;
            CHECK(attempt(s) == GPSIQ_E_DEVICE && g_error[0] != 0);                  // reported through HIP_TRY / fail
            CHECK(live_total() == k - 1);
            CHECK(attempt(s) == GPSIQ_OK);
            CHECK(live_total() == full && g_created == made + 1);                    // what was there was kept, what was missing was made
            const long before = calls_total();
            CHECK(attempt(s) == GPSIQ_OK && calls_total() == before);
        }
        reset();
    }
    std::printf("%s: %ld resources, a failure at each recovered\n", what, made);
}

// a member has a pointer and room for n elements
template <typename B>
static bool room(const B &b, size_t n) { return b.get() != nullptr && b.cap() >= n; }

// Members that share a capacity: a set that holds `small` grows to `big`, and the k-th resource that step makes fails, for every
// k.  Forget before free leaves that member empty and the ones behind it at their old size.  The next call may ask for LESS than
// the failed one (small again): it must not take the set for whole because some member still has room -- every member has a
// pointer and room for what was asked when a call returns GPSIQ_OK, here and when the set then grows to `big` after all.
// `members`: how many resources the step makes, every member `whole` names (a lone buffer that grows with slack is a group of one).
template <typename Set, typename Grow, typename Whole>
static void grow_step_recovers(const char *what, long members, Grow grow, Whole whole)
{
    const size_t small = 1000, big = 5000;
    long first = 0, step = 0;
    { Set s; CHECK(grow(s, small) == GPSIQ_OK); first = g_created; CHECK(grow(s, big) == GPSIQ_OK && whole(s, big)); step = g_created - first; CHECK(step == members); }
    reset();
    for (long k = 1; k <= step; ++k) {
        {
            Set s;
            CHECK(grow(s, small) == GPSIQ_OK && whole(s, small));
            g_fail_created_at = first + k;
            CHECK(grow(s, big) == GPSIQ_E_DEVICE);
            CHECK(grow(s, small) == GPSIQ_OK && whole(s, small));                    // asks for less than the call that failed
            const long before = calls_total();
            CHECK(grow(s, small) == GPSIQ_OK && calls_total() == before);            // and is whole: nothing left to make
            CHECK(grow(s, big) == GPSIQ_OK && whole(s, big));
        }
        reset();
    }
    std::printf("%s: a grow step of %ld resources, failed at each, recovered by a smaller request\n", what, step);
}

// reserve_together itself, on a group of three of both kinds: at or below the SMALLEST capacity no call at all; above it every
// member gets `cap`, in the order given; with the k-th allocation of the step failing, a later and smaller request completes the group
static void group_grows_together()
{
    using gpsiq::reserve_together;
    {
        DevBuf<double> a; PinnedBuf<int> b; DevBuf<uint8_t> c;
        CHECK(reserve_together(0, 64, a, b, c) == hipSuccess && calls_total() == 0);             // nothing asked for, nothing done
        CHECK(reserve_together(100, 130, a, b, c) == hipSuccess);
        CHECK(a.cap() == 130 && b.cap() == 130 && c.cap() == 130 && f_malloc.calls == 2 && f_hmalloc.calls == 1 && g_last_bytes == 130);   // c last
        long before = calls_total();
        for (size_t n : {(size_t) 130, (size_t) 100, (size_t) 1, (size_t) 0}) CHECK(reserve_together(n, n + 1000, a, b, c) == hipSuccess);
        CHECK(calls_total() == before);
        CHECK(b.reserve(500) == hipSuccess);                                                     // one member ahead of the others ...
        before = calls_total();
        CHECK(reserve_together(130, 999, a, b, c) == hipSuccess && calls_total() == before);     // ... the smallest capacity still decides
        CHECK(reserve_together(131, 200, a, b, c) == hipSuccess && a.cap() == 200 && b.cap() == 500 && c.cap() == 200);
        DevBuf<double> lone;
        CHECK(reserve_together(10, 26, lone) == hipSuccess && lone.cap() == 26 && reserve_together(26, 99, lone) == hipSuccess && lone.cap() == 26);
    }
    reset();
    for (long k = 1; k <= 3; ++k) {
        {
            DevBuf<double> a; PinnedBuf<int> b; DevBuf<uint8_t> c;
            CHECK(reserve_together(1000, 1100, a, b, c) == hipSuccess);
            g_fail_created_at = 3 + k;
            CHECK(reserve_together(5000, 5100, a, b, c) == hipErrorOutOfMemory);                 // the first error is the one returned
            CHECK((k == 1 ? a.cap() : k == 2 ? b.cap() : c.cap()) == 0 && g_created == 3 + k);   // ... and nothing behind it was touched
            CHECK(reserve_together(1000, 1100, a, b, c) == hipSuccess && room(a, 1000) && room(b, 1000) && room(c, 1000));
            const long before = calls_total();
            CHECK(reserve_together(1000, 1100, a, b, c) == hipSuccess && calls_total() == before);
        }
        reset();
    }
    std::printf("group: a grow step of 3 members, failed at each, recovered by a smaller request\n");
}

int main()
{
    grows_only<DevBuf<double>>(f_malloc, f_free);
    grows_only<PinnedBuf<gpsiq_patch_t>>(f_hmalloc, f_hfree);
    survives_failed_allocation<DevBuf<double>>(f_malloc, f_free);
    survives_failed_allocation<PinnedBuf<gpsiq_patch_t>>(f_hmalloc, f_hfree);
    survives_failed_free<DevBuf<double>>(f_malloc, f_free, 0);
    survives_failed_free<PinnedBuf<gpsiq_patch_t>>(f_hmalloc, f_hfree, 1);
    { PinnedBuf<int> b; CHECK(b.reserve(1) == hipSuccess && g_last_flags == hipHostMallocDefault); }
    reset();
    ensure_is_idempotent();
    group_grows_together();
    first_use_recovers<gpsiq_ctx::Chain>("chain", [](gpsiq_ctx::Chain &k) { return k.reserve(1000); });
    first_use_recovers<gpsiq_ctx::EvalDev>("device evaluation", [](gpsiq_ctx::EvalDev &e) { return e.reserve(1000, true, true); });
    first_use_recovers<gpsiq_ctx::EvalDev>("repair", [](gpsiq_ctx::EvalDev &e) { return e.reserve_repair(300); });
    first_use_recovers<DespreadSet>("despread", [](DespreadSet &d) { return d.reserve(1000, 1000, 1000); });
    first_use_recovers<PackSet>("pack", [](PackSet &p) { return p.reserve(); });
    first_use_recovers<PieceRing>("piece ring", [](PieceRing &r) { return r.reserve(1000, 1000); });
    first_use_recovers<AcquireSet>("acquire", [](AcquireSet &a) { return a.reserve(1000, 1000, 1000, 1000); });
    first_use_recovers<FollowSet>("follow", [](FollowSet &f) { return f.reserve(1000); });
    grow_step_recovers<gpsiq_ctx::Chain>("chain", 5, [](gpsiq_ctx::Chain &k, size_t n) { return k.reserve(n); }, [](const gpsiq_ctx::Chain &k, size_t n) {
        return room(k.d_in, n) && room(k.h_in, n) && room(k.d_prep, n * k.kPrepBytes) && room(k.d_maps, n) && room(k.h_maps, n); });
    grow_step_recovers<gpsiq_ctx::EvalDev>("device evaluation", 4, [](gpsiq_ctx::EvalDev &e, size_t n) { return e.reserve(n, true, true); },
        [](const gpsiq_ctx::EvalDev &e, size_t n) { return room(e.d_chan, n * e.kChanBytes) && room(e.h_chan, n * e.kChanBytes) && room(e.d_raw, n) && room(e.d_seeds, n); });
    grow_step_recovers<gpsiq_ctx::EvalDev>("repair", 4, [](gpsiq_ctx::EvalDev &e, size_t n) { return e.reserve_repair(n); }, [](const gpsiq_ctx::EvalDev &e, size_t n) {
        return room(e.d_slot, n) && room(e.h_slot, n) && room(e.d_col, n) && room(e.h_col, n); });
    grow_step_recovers<DespreadSet>("despread", 6, [](DespreadSet &d, size_t n) { return d.reserve(n, n, n); }, [](const DespreadSet &d, size_t n) {
        return room(d.d_sums, n) && room(d.h_sums, n) && room(d.d_prn, n) && room(d.h_prn, n) && room(d.d_stats, n) && room(d.h_stats, n); });
    grow_step_recovers<PieceRing>("piece ring", 4, [](PieceRing &r, size_t n) { return r.reserve(n, n); }, [](const PieceRing &r, size_t n) {
        return r.stage_stream.get() && r.copy_stream.get() && room(r.d_render[0], n) && room(r.d_render[1], n) && room(r.d_out[0], n) && room(r.d_out[1], n); });
    grow_step_recovers<AcquireSet>("acquire", 5, [](AcquireSet &a, size_t n) { return a.reserve(n, n, n, n); }, [](const AcquireSet &a, size_t n) {
        return room(a.d_prn, 32) && room(a.h_prn, 32) && room(a.d_power, n) && room(a.d_peaks, n) && room(a.h_peaks, n) && room(a.d_corr, n) && room(a.d_planes, n); });
    grow_step_recovers<FollowSet>("follow", 1, [](FollowSet &f, size_t n) { return f.reserve(n); }, [](const FollowSet &f, size_t n) {
        return room(f.d_state, 32) && room(f.h_state, 32) && room(f.d_count, 32) && room(f.h_count, 32) && room(f.d_epochs, n); });
    // the sizes a grown stage set ends with are each site's own: n + n/4 + 256, but + 16 for the stream statistics and + 64 for peaks and records
    {
        DespreadSet d; AcquireSet a; FollowSet f; PieceRing p;
        CHECK(d.reserve(5000, 5000, 5000) == GPSIQ_OK && a.reserve(5000, 5000, 5000, 5000) == GPSIQ_OK && f.reserve(5000) == GPSIQ_OK && p.reserve(5000, 5000) == GPSIQ_OK);
        const size_t base = 5000 + 5000 / 4;
        CHECK(d.d_sums.cap() == base + 256 && d.h_sums.cap() == base + 256 && d.d_prn.cap() == base + 256 && d.h_prn.cap() == base + 256);
        CHECK(d.d_stats.cap() == base + 16 && d.h_stats.cap() == base + 16);
        CHECK(a.d_power.cap() == base + 256 && a.d_peaks.cap() == base + 64 && a.h_peaks.cap() == base + 64 && a.d_corr.cap() == base + 256 && a.d_planes.cap() == base + 256);
        CHECK(f.d_epochs.cap() == base + 64);
        CHECK(p.d_render[0].cap() == base + 256 && p.d_render[1].cap() == base + 256 && p.d_out[0].cap() == base + 256 && p.d_out[1].cap() == base + 256);
        PackSet q;                                                                   // the packer's own: the counter and its timing events
        CHECK(q.reserve() == GPSIQ_OK && room(q.clip.d_count, 1) && room(q.clip.h_count, 1) && q.clip.t0.get() && q.clip.t1.get());
        PieceRing m;                                                                 // a stage that works in place: no output pair
        CHECK(m.reserve(100, 0) == GPSIQ_OK && room(m.d_render[0], 100) && room(m.d_render[1], 100) && !m.d_out[0].get() && !m.d_out[1].get());
        AcquireSet g;                                                                // the generic kernel without correlations: neither buffer made
        CHECK(g.reserve(100, 10, 0, 0) == GPSIQ_OK && !g.d_corr.get() && !g.d_planes.get() && room(g.d_power, 100));
    }
    reset();
    // the sizes a grown chain ends with are the policy's, and at or below them nothing is called
    {
        gpsiq_ctx::Chain k;
        CHECK(k.reserve(1000) == GPSIQ_OK && k.reserve(5000) == GPSIQ_OK);
        const size_t cap = 5000 + 5000 / 4 + 256;
        CHECK(k.d_in.cap() == cap && k.h_in.cap() == cap && k.d_prep.cap() == cap * k.kPrepBytes && k.d_maps.cap() == cap && k.h_maps.cap() == cap);
        const long before = calls_total();
        CHECK(k.reserve(cap) == GPSIQ_OK && k.reserve(1) == GPSIQ_OK && calls_total() == before);
    }
    reset();
    // a whole context is torn down by its members: every stream and event gpsiq_create makes, a buffer of each owner
    {
        gpsiq_ctx c;
        CHECK(c.stream.ensure() == hipSuccess && c.copy_stream[1].ensure() == hipSuccess && c.chunk_done[0].ensure() == hipSuccess);
        CHECK(c.d_tab.reserve(1) == hipSuccess && c.buf[2].h_patch.reserve(256) == hipSuccess && c.aslot[3].out.reserve(16) == hipSuccess);
        CHECK(c.buf[0].use[3].ev.ensure() == hipSuccess && c.d_noise_tab.reserve(4) == hipSuccess && c.d_zero_tab.reserve(4) == hipSuccess);
        CHECK(c.chain.reserve(10) == GPSIQ_OK && c.evd.reserve(10, false, false) == GPSIQ_OK);
        CHECK(c.dsp.reserve(10, 10, 1) == GPSIQ_OK && c.pack.reserve() == GPSIQ_OK && c.ring.reserve(10, 10) == GPSIQ_OK && c.acq.reserve(10, 10, 10, 10) == GPSIQ_OK && c.fol.reserve(10) == GPSIQ_OK);
    }
    reset();
    std::printf("own types ok\n");
    return 0;
}
