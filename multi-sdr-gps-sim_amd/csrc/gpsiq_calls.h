// gpsiq_calls.h -- what the host threads of one batch call share (gpsiq_batch.cpp, gpsiq_multi.cpp): the outcome of a part of the
// call, the queue of pieces between the thread that feeds a device and the thread that renders on it, and the walk's helper thread.
// Host code only, no HIP: tests/sanitize_refwalk.cpp runs them under ThreadSanitizer.
#ifndef GPSIQ_CALLS_H
#define GPSIQ_CALLS_H

#include <condition_variable>
#include <deque>
#include <mutex>

#include "gpsiq_internal.h"

namespace gpsiq {

// The outcome of a part of a call that runs beside others: the first error it met, code and text (the text of
// gpsiq_last_error() belongs to the thread that failed, and the next failure on that thread overwrites it).  One thread takes
// errors; others may poll ok() while it runs, and read the text once it has been joined.
struct Status {
    bool ok() const { return rc.load(std::memory_order_acquire) == GPSIQ_OK; }
    int  code() const { return rc.load(std::memory_order_acquire); }
    // code != GPSIQ_OK and nothing held yet: hold it with `what` (default: this thread's gpsiq_last_error())
    void take(int code_, const char *what = nullptr)
    {
        if (code_ == GPSIQ_OK || !ok()) return;
        std::snprintf(text, sizeof text, "%s", what ? what : gpsiq_last_error());
        rc.store(code_, std::memory_order_release);
    }
    int fail() const { return set_error(code(), text); }      // the calling thread's error is what is held here
    char text[400] = "";
private:
    std::atomic<int> rc{GPSIQ_OK};
};

// Items from one thread to another, in order; close() says that no more will come.
template <typename T> struct WorkQueue {
    void push(T &&item)
    {
        { std::lock_guard<std::mutex> lock(mu); items.push_back(std::move(item)); }
        cv.notify_one();
    }
    void close()
    {
        { std::lock_guard<std::mutex> lock(mu); closed = true; }
        cv.notify_one();
    }
    bool pop(T *out)                                           // waits for an item; false: closed, and nothing left
    {
        std::unique_lock<std::mutex> lock(mu);
        cv.wait(lock, [this] { return !items.empty() || closed; });
        if (items.empty()) return false;
        *out = std::move(items.front());
        items.pop_front();
        return true;
    }
private:
    std::mutex mu;
    std::condition_variable cv;
    std::deque<T> items;
    bool closed = false;
};

// The reference walk driven by a helper thread of its own while the thread that made it renders the pieces; where none can be
// started (or own_thread is false: a single piece) the walk runs here, before anything is rendered.  Declared behind the walk:
// the walkers read the caller's descriptors and write its q, and are never left running.
struct WalkThread {
    explicit WalkThread(RefWalk &w, bool own_thread = true)
    {
        started = own_thread && pthread_create(&th, nullptr, [](void *p) -> void * { static_cast<RefWalk *>(p)->run(); return nullptr; }, &w) == 0;
        if (!started) w.run();
    }
    void join() { if (started) pthread_join(th, nullptr); started = false; }
    ~WalkThread() { join(); }
    WalkThread(const WalkThread &) = delete;
    WalkThread &operator=(const WalkThread &) = delete;
private:
    pthread_t th;
    bool started = false;
};

}  // namespace gpsiq
#endif
