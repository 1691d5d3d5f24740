// The one owner of a recycled block: frees what it holds when it is destroyed, reset or assigned over, so that no owner keeps a
// free list by hand.  Plain C++ (no HIP include): tests/owned_block_host.cpp instantiates it with a counting free function.
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
