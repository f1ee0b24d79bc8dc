// gpsiq_own.h -- what the device context (gpsiq_ctx.h) is made of: device memory, page-locked host memory, events and streams
// that own themselves.  Host code only.  Every type is non-copyable and gives its resource back in its destructor, so a context
// is torn down by `delete` and a member cannot be forgotten.  Nothing here reports an error by itself: every call returns the
// hipError_t of the runtime call that failed, for the caller's HIP_TRY (below: the routines built from these types use it, in
// gpsiq_ctx.h and in the stage headers it includes).
#ifndef GPSIQ_OWN_H
#define GPSIQ_OWN_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace gpsiq {

int fail(int code, const char *fmt, ...);                // gpsiq_internal.h; libgpsiq's error text of the calling thread

// (GPSIQ_E_DEVICE: include/gpsiq.h, which every file that expands the macro has seen)
#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return gpsiq::fail(GPSIQ_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

// Memory that only grows.  reserve(count): at or below the capacity an inline compare and nothing else.  To grow, the pointer is
// FORGOTTEN and the capacity zeroed before the old allocation is freed, and the new one is counted only once it exists: whichever
// step fails, the buffer is left empty -- never holding a pointer that has been freed, never claiming room it does not have -- and
// the next reserve() starts over.  (The free is hipFree / hipHostFree itself, not an asynchronous one: it waits for whatever
// still uses the old allocation, and callers that grow a buffer with work in flight rely on that.)  The contents are not kept.
template <typename T, bool kPinned>
class Buf {
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { if (p_) (void) release(p_); }
    T *get() const { return p_; }
    size_t cap() const { return cap_; }                  // in elements
    T &operator[](size_t i) const                        // page-locked memory only: a device pointer is not the host's to follow
    {
        static_assert(kPinned, "operator[] on device memory");
        return p_[i];
    }
    hipError_t reserve(size_t count) { return count <= cap_ ? hipSuccess : grow(count); }
private:
    static hipError_t release(void *p) { return kPinned ? hipHostFree(p) : hipFree(p); }
    hipError_t grow(size_t count)
    {
        T *old = p_;
        p_ = nullptr; cap_ = 0;
        hipError_t e = old ? release(old) : hipSuccess;
        void *fresh = nullptr;
        if (e == hipSuccess) e = kPinned ? hipHostMalloc(&fresh, count * sizeof(T), hipHostMallocDefault) : hipMalloc(&fresh, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(fresh); cap_ = count;
        return hipSuccess;
    }
    T     *p_ = nullptr;
    size_t cap_ = 0;
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

// First use and growth of a set of resources.  Every member is ensured / reserved by every call, each a compare once it exists: a
// call that fails part-way returns its error, and the next call makes what is still missing instead of taking a half-made set for
// a whole one.  Members that share a capacity (a device buffer and its page-locked staging; a lone buffer that grows with slack is a
// group of one) are grown in one step that is entered while ANY of them lacks room for `need` (the smallest of their capacities):
// after a step that failed part-way -- forget before free leaves the member it failed at empty, the ones behind it at their old
// size -- every later call enters it again, whatever its need.  The step reserves `cap` (the caller's: need plus its slack) in every
// member, in the order given, and returns the first error.
template <typename... B>
hipError_t reserve_together(size_t need, size_t cap, B &...bufs)
{
    if (need <= std::min({bufs.cap()...})) return hipSuccess;
    hipError_t e = hipSuccess;
    (void) (((e = bufs.reserve(cap)) == hipSuccess) && ...);
    return e;
}

// ensure(): creates the event on first use, does nothing after that.  hipEventDefault for the events whose times are read.
class Event {
public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e_) (void) hipEventDestroy(e_); }
    hipEvent_t get() const { return e_; }
    hipError_t ensure(unsigned flags = hipEventDisableTiming) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
private:
    hipEvent_t e_ = nullptr;
};

// ensure(): a non-blocking stream on first use; ensure_greatest(): one of the device's greatest priority.
class Stream {
public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s_) (void) hipStreamDestroy(s_); }
    hipStream_t get() const { return s_; }
    hipError_t ensure() { return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
    hipError_t ensure_greatest()
    {
        if (s_) return hipSuccess;
        int least = 0, greatest = 0;
        (void) hipDeviceGetStreamPriorityRange(&least, &greatest);
        return hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, greatest);
    }
private:
    hipStream_t s_ = nullptr;
};

}  // namespace gpsiq
#endif
