// mem_driver.cc -- csrc/bp_mem.h on its own (no HIP, no library): counting stand-ins for the handful of runtime calls the header
// uses, then the header.  Checks the grow-only policy, that a request that fits makes no call, that streams are synchronised
// before a free and only then, that allocations and frees balance (scope exit, moves, a failing allocation in the middle of a
// multi-buffer grow), the same for events and streams, and Layout against the hand-written al256 chain.  Built with
// -fsanitize=address,undefined: every stand-in allocation is a heap block of its exact size, so a holder that forgets one is a
// leak report and one that frees twice or early ends the run.  Exits non-zero with a message on the first mismatch.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

// ---- the stand-ins
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct StreamTag *hipStream_t;
typedef struct EventTag *hipEvent_t;

static std::vector<std::string> g_log;        // every runtime call, in order
static int g_dev = 0, g_pin = 0, g_ev = 0, g_st = 0;   // live device blocks, pinned blocks, events, streams
static int g_fail_in = -1;                    // >= 0: that many more allocations succeed, then one fails
static size_t g_last_bytes = 0;

static bool alloc_fails()
{
    if (g_fail_in < 0) return false;
    return g_fail_in-- == 0;
}
static std::string ptr_name(const void *p) { char b[32]; snprintf(b, sizeof b, "%p", p); return b; }
static hipError_t hipMalloc(void **p, size_t n)
{
    if (alloc_fails()) { g_log.push_back("malloc-fail"); *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(n); g_last_bytes = n; ++g_dev; g_log.push_back("malloc");
    return hipSuccess;
}
static hipError_t hipHostMalloc(void **p, size_t n)
{
    if (alloc_fails()) { g_log.push_back("hostmalloc-fail"); *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(n); g_last_bytes = n; ++g_pin; g_log.push_back("hostmalloc");
    return hipSuccess;
}
static hipError_t hipFree(void *p) { free(p); --g_dev; g_log.push_back("free"); return hipSuccess; }
static hipError_t hipHostFree(void *p) { free(p); --g_pin; g_log.push_back("hostfree"); return hipSuccess; }
static hipError_t hipStreamSynchronize(hipStream_t s) { g_log.push_back("sync " + ptr_name(s)); return hipSuccess; }
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)malloc(1); ++g_ev; g_log.push_back("evcreate"); return hipSuccess; }
static hipError_t hipEventDestroy(hipEvent_t e) { free(e); --g_ev; g_log.push_back("evdestroy"); return hipSuccess; }
static hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)malloc(1); ++g_st; g_log.push_back("stcreate"); return hipSuccess; }
static hipError_t hipStreamDestroy(hipStream_t s) { free(s); --g_st; g_log.push_back("stdestroy"); return hipSuccess; }
static const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }

#include "bp_mem.h"

thread_local std::string g_bp_err;

#define FAIL(...) do { printf("mem_driver: line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)
#define CHECK(c) do { if (!(c)) FAIL("%s", #c); } while (0)

static void expect_log(size_t from, std::vector<std::string> want, int line)
{
    std::vector<std::string> got(g_log.begin() + from, g_log.end());
    if (got == want) return;
    printf("mem_driver: line %d: calls were:", line);
    for (auto &s : got) printf(" [%s]", s.c_str());
    printf("\n");
    exit(1);
}
#define EXPECT_LOG(from, ...) expect_log(from, {__VA_ARGS__}, __LINE__)

static const hipStream_t S1 = (hipStream_t)0x10, S2 = (hipStream_t)0x20;
static size_t policy(size_t n) { return n + n / 4 + 4096; }       // the growth policy, restated

static void test_grow_policy()
{
    const std::string s1 = "sync " + ptr_name(S1), s2 = "sync " + ptr_name(S2);
    for (int pin = 0; pin < 2; ++pin) {
        const char *M = pin ? "hostmalloc" : "malloc", *F = pin ? "hostfree" : "free";
        size_t at = g_log.size();
        {
            Buf b;
            CHECK(b.grow(0, pin, "x: ", {S1, S2}) == BP_OK);                 // 0 bytes: nothing is allocated, p stays as it was
            CHECK(b.p == nullptr && b.bytes == 0);
            EXPECT_LOG(at);
            CHECK(b.grow(1, pin, "x: ", {S1, S2}) == BP_OK);                 // the first allocation: nothing to wait for
            CHECK(b.p && b.bytes == 4097 && g_last_bytes == 4097);
            EXPECT_LOG(at, M);
            memset(b.p, 0x5a, b.bytes);                                      // (all of it is there)
            void *p0 = b.p;
            at = g_log.size();
            for (size_t n : {(size_t)4096, (size_t)4097, (size_t)17, (size_t)0}) {   // they fit: no call at all
                CHECK(b.grow(n, pin, "x: ", {S1, S2}) == BP_OK);
                CHECK(b.p == p0 && b.bytes == 4097);
            }
            EXPECT_LOG(at);
            const size_t big = b.bytes + b.bytes / 4 + 4097;                 // past 1.25 x capacity + 4096
            CHECK(b.grow(big, pin, "x: ", {S1, S2}) == BP_OK);
            CHECK(b.bytes == policy(big) && b.bytes == 9218 + 2304 + 4096 && g_last_bytes == b.bytes);
            EXPECT_LOG(at, s1, s2, F, M);                                    // the streams, then the free, then the allocation
            memset(b.p, 0x5a, b.bytes);
            at = g_log.size();
            CHECK(b.grow(b.bytes + 1, pin, "x: ", {}) == BP_OK);             // (no stream to wait for)
            EXPECT_LOG(at, F, M);
            at = g_log.size();
        }
        EXPECT_LOG(at, F);                                                   // scope exit
        CHECK(g_dev == 0 && g_pin == 0);
        for (size_t n : {(size_t)4096, (size_t)4097, (size_t)1000000}) {     // fresh buffers
            Buf b;
            CHECK(b.grow(n, pin, "x: ", {S1}) == BP_OK && b.bytes == policy(n) && b.pinned == (pin != 0));
        }
        CHECK(g_dev == 0 && g_pin == 0);
    }
    CHECK(policy(4096) == 9216 && policy(4097) == 9217);
}

static void test_alloc_and_moves()
{
    size_t at = g_log.size();
    {
        Buf a;
        CHECK(a.alloc(100) == hipSuccess && a.bytes == 100 && g_last_bytes == 100 && !a.pinned);      // exactly the bytes asked for
        CHECK(a.alloc(7, true) == hipSuccess && a.bytes == 7 && a.pinned);                             // what was held goes first
        EXPECT_LOG(at, "malloc", "free", "hostmalloc");
        CHECK(a.as<char>() == (char *)a.p);
        Buf b(std::move(a));
        CHECK(!a.p && !a.bytes && b.p && b.bytes == 7 && b.pinned);
        Buf c;
        CHECK(c.alloc(32) == hipSuccess);
        at = g_log.size();
        c = std::move(b);                                                                               // c's own block goes
        EXPECT_LOG(at, "free");
        CHECK(!b.p && c.bytes == 7 && c.pinned && g_dev == 0 && g_pin == 1);
        std::vector<Buf> v;
        for (int k = 0; k < 9; ++k) { Buf q; CHECK(q.alloc(8 + k) == hipSuccess); v.push_back(std::move(q)); }   // (reallocating vector)
        CHECK(g_dev == 9);
        at = g_log.size();
        c.release(); c.release();
        EXPECT_LOG(at, "hostfree");
    }
    CHECK(g_dev == 0 && g_pin == 0);
    {
        Buf a;                                                                                          // a failing exact allocation
        g_fail_in = 0;
        CHECK(a.alloc(64) != hipSuccess && !a.p && !a.bytes);
        g_fail_in = -1;
    }
    CHECK(g_dev == 0 && g_pin == 0);
}

static void test_grow_all()
{
    Buf a, b, c, d;
    CHECK(grow_all("t: ", {S1}, {{a, 10, false}, {b, 0, false}, {c, 30, true}, {d, 40, false}}) == BP_OK);
    CHECK(a.bytes == policy(10) && !b.p && c.bytes == policy(30) && c.pinned && d.bytes == policy(40));
    CHECK(g_dev == 2 && g_pin == 1);
    void *pd = d.p;
    const size_t at = g_log.size();
    CHECK(grow_all("t: ", {S1}, {{a, 10, false}, {b, 0, false}, {c, 30, true}, {d, 40, false}}) == BP_OK);   // everything fits
    EXPECT_LOG(at);
    // the third allocation fails: a and b have grown and stay valid, c is empty, d was not reached and keeps what it had
    g_fail_in = 2;
    g_bp_err.clear();
    const int r = grow_all("signal-layer buffers: ", {S1}, {{a, 100000, false}, {b, 5, false}, {c, 100000, true}, {d, 100000, false}});
    g_fail_in = -1;
    CHECK(r == BP_ERR_NOMEM);
    if (g_bp_err != "signal-layer buffers: out of memory") FAIL("message '%s'", g_bp_err.c_str());
    CHECK(a.bytes == policy(100000) && b.bytes == policy(5) && !c.p && !c.bytes && d.p == pd && d.bytes == policy(40));
    memset(a.p, 1, a.bytes); memset(b.p, 2, b.bytes); memset(d.p, 3, d.bytes);
    CHECK(g_dev == 3 && g_pin == 0);
    CHECK(grow_all("t: ", {S1}, {{c, 1, true}}) == BP_OK && c.bytes == 4097);    // an empty holder grows again
    // (a, b, c, d go here: the balance is checked by the caller)
}

static void test_events_and_streams()
{
    const size_t at = g_log.size();
    {
        Event e, unused;
        Stream s, none;
        CHECK(e.create() == hipSuccess && s.create(1) == hipSuccess);
        CHECK((hipEvent_t)e != nullptr && (hipStream_t)s != nullptr && (hipEvent_t)unused == nullptr && (hipStream_t)none == nullptr);
        std::vector<Event> v;
        for (int k = 0; k < 9; ++k) { Event q; CHECK(q.create(2) == hipSuccess); v.push_back(std::move(q)); }
        CHECK(g_ev == 10 && g_st == 1);
    }
    CHECK(g_ev == 0 && g_st == 0);
    int created = 0, destroyed = 0;
    for (size_t k = at; k < g_log.size(); ++k) { created += g_log[k] == "evcreate"; destroyed += g_log[k] == "evdestroy"; }
    CHECK(created == 10 && destroyed == 10);
}

static size_t al256_again(size_t b) { return (b + 255) / 256 * 256; }        // the alignment, restated
static void test_layout()
{
    const size_t part[7] = {0, 1, 255, 256, 257, 0, 8};
    for (size_t start : {(size_t)0, (size_t)512}) {
        // the chain as it was written by hand: each offset is the one before it plus the aligned size of the part before it
        const size_t o0 = start, o1 = o0 + al256_again(part[0]), o2 = o1 + al256_again(part[1]), o3 = o2 + al256_again(part[2]);
        const size_t o4 = o3 + al256_again(part[3]), o5 = o4 + al256_again(part[4]), o6 = o5 + al256_again(part[5]);
        const size_t total = o6 + al256_again(part[6]);
        const size_t want[7] = {o0, o1, o2, o3, o4, o5, o6};
        Layout lay(start);
        for (int k = 0; k < 7; ++k) {
            const size_t o = lay.take(part[k]);
            if (o != want[k]) FAIL("part %d at %zu, the chain says %zu", k, o, want[k]);
        }
        CHECK(lay.size() == total);
        CHECK(want[0] == want[1] && want[5] == want[6]);                     // a part of 0 bytes shares its offset with the next
        CHECK(total == start + 256 + 256 + 256 + 512 + 256);
    }
    CHECK(Layout().size() == 0);
    for (size_t b : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, ((size_t)1 << 33) + 1}) CHECK(al256(b) == al256_again(b));
}

int main()
{
    test_grow_policy();
    test_alloc_and_moves();
    test_grow_all();
    CHECK(g_dev == 0 && g_pin == 0);
    test_events_and_streams();
    test_layout();
    CHECK(g_dev == 0 && g_pin == 0 && g_ev == 0 && g_st == 0);
    printf("mem_driver: holders balance, grow policy and layout agree (%zu runtime calls)\n", g_log.size());
    return 0;
}
