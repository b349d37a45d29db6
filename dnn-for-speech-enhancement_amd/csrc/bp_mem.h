// bp_mem.h -- who frees what: scoped holders of device memory, pinned host memory, events and streams, the grow-only policy
// of the library's buffers, and the running offsets of a block's parts.  With them: the error plumbing every unit uses (fail,
// HIPCHK).  Internal: nothing in here is part of the C ABI.  Like the host part of bp_stream_core.h this header names the HIP
// runtime's calls but includes no HIP header: the units include <hip/hip_runtime.h> first, the test program
// (tests/cpp/mem_driver.cc) stands counting functions in for them.
#pragma once
#include <stddef.h>

#include <initializer_list>
#include <string>
#include <utility>

#include "../../include/bp_c_api.h"

extern thread_local std::string g_bp_err;
static inline int fail(int code, const std::string &msg) { g_bp_err = msg; return code; }
#define HIPCHK(x)                                                                                     \
    do {                                                                                              \
        hipError_t _e = (x);                                                                          \
        if (_e != hipSuccess)                                                                         \
            return fail(BP_ERR_DEVICE, std::string(#x) + ": " + hipGetErrorString(_e));               \
    } while (0)

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }   // the parts of a device block start 256-byte aligned

// The parts of one block, in order: take() hands out where a part starts and moves on by its aligned size (a part of 0 bytes
// takes no room and shares its offset with the next one); size() is the block's size so far.
struct Layout {
    size_t at;
    explicit Layout(size_t start = 0) : at(start) {}
    size_t take(size_t bytes) { const size_t o = at; at += al256(bytes); return o; }
    size_t size() const { return at; }
};

// One allocation, device or pinned host (which: said by the call that allocates), freed when the holder goes.
struct Buf {
    void *p = nullptr;
    size_t bytes = 0;            // capacity
    bool pinned = false;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), bytes(o.bytes), pinned(o.pinned) { o.p = nullptr; o.bytes = 0; }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; pinned = o.pinned; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~Buf() { release(); }
    template <class T> T *as() const { return static_cast<T *>(p); }
    void release()
    {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; bytes = 0;
    }
    // exactly n bytes (what was held goes first)
    hipError_t alloc(size_t n, bool pin = false)
    {
        release();
        pinned = pin;
        const hipError_t e = pin ? hipHostMalloc(&p, n) : hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    // Grow-only: a request that fits costs nothing, no call and no synchronisation (the fast path of every push and every
    // training call; a request of 0 bytes always fits).  Otherwise the streams that may still use the old allocation are
    // synchronised, it is freed and n + 25 % + 4096 bytes are allocated; BP_ERR_NOMEM "<what><hip error string>" if that fails,
    // and the holder is then empty.
    int grow(size_t n, bool pin, const char *what, std::initializer_list<hipStream_t> sync)
    {
        if (n <= bytes) return BP_OK;
        return regrow(n, pin, what, sync);
    }

private:
    int regrow(size_t n, bool pin, const char *what, std::initializer_list<hipStream_t> sync)
    {
        if (p) {
            for (hipStream_t st : sync) HIPCHK(hipStreamSynchronize(st));
            release();
        }
        const hipError_t e = alloc(n + n / 4 + 4096, pin);
        return e == hipSuccess ? BP_OK : fail(BP_ERR_NOMEM, std::string(what) + hipGetErrorString(e));
    }
};

// Several grow-only buffers in one statement, grown in the order written; the first error ends it, and what grew before it
// stays valid.
struct Grow { Buf &b; size_t bytes; bool pinned; };
static inline int grow_all(const char *what, std::initializer_list<hipStream_t> sync, std::initializer_list<Grow> list)
{
    for (const Grow &g : list) {
        const int r = g.b.grow(g.bytes, g.pinned, what, sync);
        if (r != BP_OK) return r;
    }
    return BP_OK;
}

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = 0) { return hipEventCreateWithFlags(&e, flags); }   // (0: hipEventDefault, a timing event)
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s, flags); }
    operator hipStream_t() const { return s; }
};
