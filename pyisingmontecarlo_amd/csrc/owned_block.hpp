// The one owner of a recycled block: frees what it holds when it is destroyed, reset or assigned over, so that no owner keeps a
// free list by hand; below it the same for a pooled stream or event.  Plain C++ (no HIP include): tests/owned_block_host.cpp
// instantiates both with counting free functions.
#pragma once
#include <utility>

template <typename T, void (*Free)(void *)>
class OwnedBlock {
    T *p_ = nullptr;

public:
    OwnedBlock() = default;
    explicit OwnedBlock(T *p) : p_(p) {} // adopts p
    OwnedBlock(const OwnedBlock &) = delete;
    OwnedBlock &operator=(const OwnedBlock &) = delete;
    OwnedBlock(OwnedBlock &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    OwnedBlock &operator=(OwnedBlock &&o) noexcept
    {
        OwnedBlock(std::move(o)).swap(*this); // the old block goes with the temporary
        return *this;
    }
    ~OwnedBlock() { if (p_) Free(p_); }

    T *get() const { return p_; }
    operator T *() const { return p_; } // pointer arithmetic, null tests, copies and launches read as with a raw pointer
    void reset() { OwnedBlock().swap(*this); }
    void swap(OwnedBlock &o) noexcept { std::swap(p_, o.p_); }
};

// The two caches of core.hip.  Whoever drops a block has made sure first that nothing enqueued still uses it: the next request
// of that size picks it up at once.
__attribute__((visibility("hidden"))) void cached_free(void *p);
__attribute__((visibility("hidden"))) void cached_host_free(void *p);
template <typename T>
using DevBlock = OwnedBlock<T, cached_free>; // device memory
template <typename T>
using PinnedBlock = OwnedBlock<T, cached_host_free>; // pinned host memory

// The same owner for an opaque handle value H (a pointer type: a stream, an event): hands it back through Release when it is
// destroyed, reset or assigned over, and reads as the raw handle wherever one is expected.  An empty handle releases nothing.
template <typename H, void (*Release)(H)>
class OwnedHandle {
    H h_ = nullptr;

public:
    OwnedHandle() = default;
    explicit OwnedHandle(H h) : h_(h) {} // adopts h
    OwnedHandle(const OwnedHandle &) = delete;
    OwnedHandle &operator=(const OwnedHandle &) = delete;
    OwnedHandle(OwnedHandle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    OwnedHandle &operator=(OwnedHandle &&o) noexcept
    {
        OwnedHandle(std::move(o)).swap(*this); // the old value goes with the temporary
        return *this;
    }
    ~OwnedHandle() { if (h_) Release(h_); }

    H get() const { return h_; }
    operator H() const { return h_; } // launches, hipEventRecord and null tests read as with a raw handle
    void reset() { OwnedHandle().swap(*this); }
    void swap(OwnedHandle &o) noexcept { std::swap(h_, o.h_); }
};

// The stream and event pools of core.hip (hipStream_t and hipEvent_t are pointers to these two types).  An event's kind -- with
// timing for the *_timed entry point, without for ordering between streams -- is part of its handle's type, fixed once where the
// member is declared: it cannot go back into the other kind's pool.  Released with the owner's device current and, for a
// stream, with nothing of the owner's still running on it.
struct ihipStream_t;
struct ihipEvent_t;
__attribute__((visibility("hidden"))) void pooled_stream_destroy(ihipStream_t *st);
__attribute__((visibility("hidden"))) void pooled_event_destroy(ihipEvent_t *ev, bool disable_timing);
template <bool DisableTiming>
inline void pooled_event_release(ihipEvent_t *ev) { pooled_event_destroy(ev, DisableTiming); }
using PooledStream = OwnedHandle<ihipStream_t *, pooled_stream_destroy>;
using PooledEvent = OwnedHandle<ihipEvent_t *, pooled_event_release<true>>; // no timing
using TimedEvent = OwnedHandle<ihipEvent_t *, pooled_event_release<false>>;
