// kmc_mem.hip.h -- who owns device and pinned host memory (internal, not installed).  The only file of the library that
// calls the runtime's allocator: mem_alloc and mem_free below.  Everything else holds a Mem<T> (or a struct made of
// them), which frees what it owns when it goes away and cannot be copied.  No owner has static or thread-local storage:
// a free after the runtime has shut down can crash at exit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <utility>

#include <hip/hip_runtime.h>

#pragma GCC visibility push(hidden)

// what kmc_debug_mem reports: bytes are what was asked of the allocator (defined in kmc_api.hip)
struct MemStats {
    std::atomic<uint64_t> dev_live{0}, pin_live{0};     // bytes allocated and not yet freed
    std::atomic<uint64_t> dev_allocs{0}, pin_allocs{0}; // successful allocation calls
    std::atomic<uint64_t> free_failed{0};               // frees for which the runtime returned an error
};
extern MemStats g_mem;

inline hipError_t mem_alloc(void** p, size_t bytes, bool pinned) {
    const hipError_t e = pinned ? hipHostMalloc(p, bytes) : hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; return e; }
    (pinned ? g_mem.pin_live : g_mem.dev_live) += bytes;
    (pinned ? g_mem.pin_allocs : g_mem.dev_allocs) += 1;
    return hipSuccess;
}

inline hipError_t mem_free(void* p, size_t bytes, bool pinned) {
    const hipError_t e = pinned ? hipHostFree(p) : hipFree(p);
    if (e != hipSuccess) g_mem.free_failed += 1;
    (pinned ? g_mem.pin_live : g_mem.dev_live) -= bytes;
    return e;
}

// `bytes` of device (PINNED: pinned host) memory, read as T*.  Move-only; a moved-from owner is empty.
template <typename T, bool PINNED = false>
struct Mem {
    T* p = nullptr;
    size_t bytes = 0;

    Mem() = default;
    Mem(const Mem&) = delete;
    Mem& operator=(const Mem&) = delete;
    Mem(Mem&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    Mem& operator=(Mem&& o) noexcept {
        if (this != &o) { (void)reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~Mem() { (void)reset(); }

    operator T*() const { return p; }
    T* operator->() const { return p; }

    // frees what it held first, also when the allocation then fails
    hipError_t alloc(size_t nbytes) {
        const hipError_t e = reset();
        if (e != hipSuccess) return e;
        void* q = nullptr;
        const hipError_t a = mem_alloc(&q, nbytes, PINNED);
        if (a == hipSuccess) { p = (T*)q; bytes = nbytes; }
        return a;
    }
    hipError_t reset() {
        if (!p) { bytes = 0; return hipSuccess; }
        const hipError_t e = mem_free((void*)p, bytes, PINNED);
        p = nullptr;
        bytes = 0;
        return e;
    }
};

template <typename T> using Dev = Mem<T, false>;
template <typename T> using Pin = Mem<T, true>;

#pragma GCC visibility pop
