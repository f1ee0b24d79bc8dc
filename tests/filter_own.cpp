// filter_own.cpp -- FirSet::reserve (csrc/gpsiq_filter.h), the first-use routine of the filter stage's member of the device
// context, and with it PieceRing::reserve (csrc/gpsiq_stage_batch.h), the staging ring the filtered batch call works through its
// pieces with, on the CPU, in the manner of tests/own_types.cpp.  `Both` below is what that call reserves: its sixteen resources.
// TEST INFRASTRUCTURE: tests/test_filter_own.py builds this file with the address and undefined-behaviour sanitizers and runs it.
// No HIP runtime is linked: the entry points gpsiq_own.h calls are counting fakes over malloc / free that share one sequence number,
// so that "the k-th resource the routine makes" can be made to fail whatever its kind, and that abort on a pointer they do not know.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>

#include "gpsiq_ctx.h"

namespace {

long g_created = 0, g_fail_created_at = 0, g_calls = 0;
std::set<void *> g_live;

[[noreturn]] void die(const char *what, const char *where)
{
    std::fprintf(stderr, "filter_own: %s (%s)\n", what, where);
    std::abort();
}
#define CHECK(cond) do { if (!(cond)) die("check failed: " #cond, __func__); } while (0)

hipError_t make(void **out, size_t bytes)
{
    ++g_calls;
    if (++g_created == g_fail_created_at) return hipErrorOutOfMemory;
    *out = std::malloc(bytes ? bytes : 1);
    g_live.insert(*out);
    return hipSuccess;
}
hipError_t drop(void *p, const char *name)
{
    ++g_calls;
    if (!g_live.count(p)) die("released twice, or never handed out", name);
    g_live.erase(p);
    std::free(p);
    return hipSuccess;
}
void reset()
{
    CHECK(g_live.empty());                                             // every scenario ends with nothing alive
    g_created = g_fail_created_at = g_calls = 0;
}

}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return make(p, bytes); }
hipError_t hipFree(void *p) { return drop(p, "hipFree"); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return make(p, bytes); }
hipError_t hipHostFree(void *p) { return drop(p, "hipHostFree"); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make(reinterpret_cast<void **>(e), 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop(e, "hipEventDestroy"); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return make(reinterpret_cast<void **>(s), 1); }
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { return make(reinterpret_cast<void **>(s), 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return drop(s, "hipStreamDestroy"); }
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) { *least = 1; *greatest = -2; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "fake error"; }
}

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

using gpsiq::FirSet;
using gpsiq::PieceRing;

// what gpsiq_generate_batch_filtered reserves, in its order: the ring, then the filter's own
struct Both {
    PieceRing r; FirSet f;
    int reserve(size_t render, size_t out) { if (int rc = r.reserve(render, out)) return rc; return f.reserve(); }
};

template <typename B>
static bool room(const B &b, size_t n) { return b.get() != nullptr && b.cap() >= n; }

static bool whole(const Both &b, size_t n)
{
    const FirSet &f = b.f;
    const PieceRing &r = b.r;
    return room(f.d_coef, FirSet::kCoefBytes) && room(f.h_coef, FirSet::kCoefBytes) && room(f.clip.d_count, 1) && room(f.clip.h_count, 1) &&
           room(r.d_render[0], n) && room(r.d_render[1], n) && room(r.d_out[0], n) && room(r.d_out[1], n) && r.stage_stream.get() && r.copy_stream.get() &&
           f.clip.t0.get() && f.clip.t1.get() && r.staged[0].get() && r.staged[1].get() && r.copied[0].get() && r.copied[1].get();
}

int main()
{
    // gpsiq_filter: coefficients, counter and the two timing events alone -- no stream, no staging
    {
        FirSet f;
        CHECK(f.reserve() == GPSIQ_OK && g_created == 6 && room(f.d_coef, FirSet::kCoefBytes) && room(f.clip.h_count, 1));
        const long before = g_calls;
        CHECK(f.reserve() == GPSIQ_OK && g_calls == before);
    }
    reset();
    // first use of the batch call's set: with the k-th resource failing the first attempt reports, the second completes the set --
    // nothing made twice -- and a third makes no call
    long made = 0;
    { Both f; CHECK(f.reserve(1000, 1000) == GPSIQ_OK && whole(f, 1000)); made = g_created; CHECK((long) g_live.size() == made && made == 16); }
    reset();
    for (long k = 1; k <= made; ++k) {
        {
            Both f;
            g_fail_created_at = k;
            g_error[0] = 0;
            CHECK(f.reserve(1000, 1000) == GPSIQ_E_DEVICE && g_error[0] != 0 && (long) g_live.size() == k - 1);
            CHECK(f.reserve(1000, 1000) == GPSIQ_OK && whole(f, 1000) && (long) g_live.size() == made && g_created == made + 1);
            const long before = g_calls;
            CHECK(f.reserve(1000, 1000) == GPSIQ_OK && g_calls == before);
        }
        reset();
    }
    std::printf("filter: %ld resources, a failure at each recovered\n", made);
    // the staging pairs grow together: a grow step that failed at any of its four allocations is completed by a later, smaller request
    for (long k = 1; k <= 4; ++k) {
        {
            Both f;
            CHECK(f.reserve(1000, 1000) == GPSIQ_OK);
            g_fail_created_at = g_created + k;
            CHECK(f.reserve(5000, 5000) == GPSIQ_E_DEVICE);
            CHECK(f.reserve(1000, 1000) == GPSIQ_OK && whole(f, 1000));
            const long before = g_calls;
            CHECK(f.reserve(1000, 1000) == GPSIQ_OK && g_calls == before);
            CHECK(f.reserve(5000, 5000) == GPSIQ_OK && whole(f, 5000));
            CHECK(f.r.d_render[0].cap() == f.r.d_render[1].cap() && f.r.d_out[0].cap() == f.r.d_out[1].cap() && f.r.d_out[0].cap() == 5000 + 5000 / 4 + 256);
        }
        reset();
    }
    std::printf("filter: a grow step of 4 resources, failed at each, recovered by a smaller request\n");
    std::printf("filter own ok\n");
    return 0;
}
