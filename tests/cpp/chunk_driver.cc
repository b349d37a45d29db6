// chunk_driver.cc -- csrc/bp_chunk.h on its own (no HIP, no library): logging stand-ins for the event and stream calls the header
// names (and counting ones for what bp_mem.h's holders need), then the header.  Checks the order of runtime calls of the upload
// handshake for a first, a second and a third upload; that interleaved stacked and window uploads wait only on their own Retire;
// that every way of making a chunk resident leaves a grown generation, no pre-staged tile and next_first -1; that the
// preconditions answer range before targets with the right status and leave the record alone; unpad_rows against poisoned pad
// columns; and the order of sq_err_sum's fp32 accumulation on sums written down by hand, through all three forms of targ_row.
// Built with -fsanitize=address,undefined.  Exits non-zero with a message on the first mismatch.
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

static std::vector<std::string> g_log;        // every stream / event call, in order
static int g_ev = 0, g_blocks = 0;            // live events, live device and pinned blocks
static std::vector<std::pair<void *, std::string>> g_names;
static void name(void *p, const char *n)      // (a freed event's address may come back: the newest name holds)
{
    for (auto &e : g_names) if (e.first == p) { e.second = n; return; }
    g_names.push_back({p, n});
}
static std::string nm(void *p)
{
    for (auto &e : g_names) if (e.first == p) return e.second;
    return "?";
}
static hipError_t hipMalloc(void **p, size_t n) { *p = malloc(n); ++g_blocks; return hipSuccess; }
static hipError_t hipHostMalloc(void **p, size_t n) { *p = malloc(n); ++g_blocks; return hipSuccess; }
static hipError_t hipFree(void *p) { free(p); --g_blocks; return hipSuccess; }
static hipError_t hipHostFree(void *p) { free(p); --g_blocks; return hipSuccess; }
static hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)malloc(1); return hipSuccess; }
static hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)malloc(1); ++g_ev; return hipSuccess; }
static hipError_t hipEventDestroy(hipEvent_t e) { free(e); --g_ev; return hipSuccess; }
static hipError_t hipStreamSynchronize(hipStream_t s) { g_log.push_back("sync " + nm(s)); return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { g_log.push_back("record " + nm(e) + " on " + nm(s)); return hipSuccess; }
static hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { g_log.push_back(nm(s) + " waits " + nm(e)); return hipSuccess; }
static const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "error"; }

#include "bp_chunk.h"

thread_local std::string g_bp_err;

#define FAIL(...) do { printf("chunk_driver: line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)
#define CHECK(c) do { if (!(c)) FAIL("%s", #c); } while (0)

static void expect_log(size_t from, std::vector<std::string> want, int line)
{
    std::vector<std::string> got(g_log.begin() + from, g_log.end());
    if (got == want) return;
    printf("chunk_driver: line %d: calls were:", line);
    for (auto &s : got) printf(" [%s]", s.c_str());
    printf("\n");
    exit(1);
}
#define EXPECT_LOG(from, ...) expect_log(from, {__VA_ARGS__}, __LINE__)

static const hipStream_t MAIN = (hipStream_t)0x10, COPY = (hipStream_t)0x20;

// a record as bp_create leaves it: everything zero, next_first -1, the three events created
static void open_record(Resident &c)
{
    c.next_first = -1;
    CHECK(c.ev_copy.create(2) == hipSuccess && c.retired.ev.create(2) == hipSuccess && c.wretired.ev.create(2) == hipSuccess);
    name((hipEvent_t)c.ev_copy, "ev_copy"); name((hipEvent_t)c.retired.ev, "retired_s"); name((hipEvent_t)c.wretired.ev, "retired_w");
}
// the shape of bp_upload_chunk (stacked) and of upload_windows (window): begin, the copies, end, the one transition
static void upload(Resident &c, bool windows, int rows, bool has_targ)
{
    Retire &r = windows ? c.wretired : c.retired;
    int &cur = windows ? c.wcur : c.cur;
    CHECK(refill_begin(r, COPY) == BP_OK);
    g_log.push_back(std::string("copies into ") + (windows ? "set " : "pair ") + std::to_string(1 - cur));
    CHECK(refill_end(c, r, cur, COPY, MAIN) == BP_OK);
    make_resident(c, windows, rows, has_targ);
}

static void test_handshake_order()
{
    Resident c{};
    open_record(c);
    CHECK(!c.retired.valid && !c.wretired.valid && c.cur == 0 && c.wcur == 0);
    size_t at = g_log.size();
    upload(c, false, 10, true);               // the first: no wait on an event that was never recorded
    EXPECT_LOG(at, "copies into pair 1", "record ev_copy on copy", "sync copy", "main waits ev_copy", "record retired_s on main");
    CHECK(c.cur == 1 && c.retired.valid);     // the flip, behind everything
    for (int k = 2; k <= 3; ++k) {            // the second and the third: the retired wait in front of the first copy
        at = g_log.size();
        upload(c, false, 10, true);
        const std::string into = "copies into pair " + std::to_string(k % 2);
        EXPECT_LOG(at, "copy waits retired_s", into, "record ev_copy on copy", "sync copy", "main waits ev_copy", "record retired_s on main");
        CHECK(c.cur == k % 2);
    }
    // the same for the window side, with its own event
    at = g_log.size();
    upload(c, true, 7, false);
    EXPECT_LOG(at, "copies into set 1", "record ev_copy on copy", "sync copy", "main waits ev_copy", "record retired_w on main");
    CHECK(c.wcur == 1 && c.wretired.valid && c.cur == 1);
    at = g_log.size();
    upload(c, true, 7, false);
    EXPECT_LOG(at, "copy waits retired_w", "copies into set 0", "record ev_copy on copy", "sync copy", "main waits ev_copy", "record retired_w on main");
    CHECK(c.wcur == 0);
}

static void test_interleaved_uploads_wait_on_their_own_retire()
{
    Resident c{};
    open_record(c);
    const size_t at = g_log.size();
    const bool order[] = {false, true, true, false, true, false, false, true};
    int seen[2] = {0, 0};
    for (bool windows : order) {
        const size_t from = g_log.size();
        upload(c, windows, 5, true);
        const std::string own = windows ? "retired_w" : "retired_s", other = windows ? "retired_s" : "retired_w";
        for (size_t k = from; k < g_log.size(); ++k)
            if (g_log[k].find(other) != std::string::npos) FAIL("a %s upload touched %s: %s", windows ? "window" : "stacked", other.c_str(), g_log[k].c_str());
        CHECK((g_log[from] == "copy waits " + own) == (seen[windows] > 0));      // its own event, once it was recorded, and only then
        ++seen[windows];
    }
    // a chunk written on the device (window_adopt): no copy stream, its retire event on the main stream, the flip
    const size_t dev = g_log.size();
    CHECK(retire_and_flip(c.wretired, c.wcur, MAIN) == BP_OK);
    EXPECT_LOG(dev, "record retired_w on main");
    CHECK(c.wcur == 1 && c.cur == 0);
    CHECK(g_log.size() - at == 8 * 5 + 6 + 1);                                  // (six of the eight uploads had something to wait for)
}

static void test_every_maker_goes_through_the_one_transition()
{
    Resident c{};
    open_record(c);
    // bp_upload_chunk, upload_windows, window_adopt, bp_fill_chunk_synthetic: (windows, rows, has_targ) as each of them says it
    const struct { bool windows; int rows; bool has_targ; } makers[] = {{false, 64, true}, {false, 0, false}, {true, 33, true}, {true, 0, false}, {true, 17, false}, {false, 256, true}};
    for (auto &m : makers) {
        const unsigned gen = c.gen;
        c.pre.valid = true; c.pre.first = 32; c.pre.tile = 1; c.pre.gen = gen; c.next_first = 96;      // whatever they were before
        const int cur = c.cur, wcur = c.wcur, tile = c.stage_cur;
        make_resident(c, m.windows, m.rows, m.has_targ);
        CHECK(c.gen == gen + 1 && !c.pre.valid && c.next_first == -1);
        CHECK(c.windows == m.windows && c.frames == m.rows && c.has_targ == m.has_targ);
        CHECK(c.cur == cur && c.wcur == wcur && c.stage_cur == tile && c.pre.gen != c.gen);              // (the flip is the handshake's)
    }
    c.gen = ~0u;                                                                                       // the generation wraps, it never sticks
    make_resident(c, false, 1, true);
    CHECK(c.gen == 0u);
}

static bool same(const Resident &a, const Resident &b)
{
    return a.frames == b.frames && a.windows == b.windows && a.has_targ == b.has_targ && a.gen == b.gen && a.cur == b.cur && a.wcur == b.wcur &&
           a.stage_cur == b.stage_cur && a.next_first == b.next_first && a.pre.valid == b.pre.valid && a.pre.first == b.pre.first &&
           a.retired.valid == b.retired.valid && a.wretired.valid == b.wretired.valid;
}
static void test_preconditions()
{
    Resident c{}, was{};
    for (int windows = 0; windows < 2; ++windows) {
        make_resident(c, windows != 0, 100, false);
        c.pre.valid = true; c.next_first = 64;
        was.frames = c.frames; was.windows = c.windows; was.has_targ = c.has_targ; was.gen = c.gen; was.pre.valid = true; was.next_first = 64;
        // the range: inside, the whole chunk, empty at the end
        CHECK(resident_range(c, "f", 0, 100) == BP_OK && resident_range(c, "f", 99, 1) == BP_OK && resident_range(c, "f", 100, 0) == BP_OK);
        g_bp_err.clear();
        CHECK(resident_range(c, "bp_train_resident", 1, 100) == BP_ERR_ARG);
        if (g_bp_err != "bp_train_resident: frame range outside the resident chunk") FAIL("message '%s'", g_bp_err.c_str());
        CHECK(resident_range(c, "f", -1, 2) == BP_ERR_ARG && resident_range(c, "f", 0, -1) == BP_ERR_ARG && resident_range(c, "f", 101, 0) == BP_ERR_ARG);
        CHECK(resident_range(c, "f", 2147483647L, 2147483647L) == BP_ERR_ARG);                          // (long arithmetic: no wrap)
        CHECK(resident_range(c, "bp_grads_resident", 90, 32, "bunch") == BP_ERR_ARG);
        if (g_bp_err != "bp_grads_resident: bunch outside the resident chunk") FAIL("message '%s'", g_bp_err.c_str());
        // the targets: one fact, the kind only words the message
        CHECK(resident_targets(c, "bp_grads_resident") == BP_ERR_STATE);
        const std::string want = std::string("bp_grads_resident: the resident ") + (windows ? "window" : "stacked") + " chunk was uploaded without targets (forward / CV upload)";
        if (g_bp_err != want) FAIL("message '%s'", g_bp_err.c_str());
        // a call that fails both ways is told about the range: the callers ask for it first
        int r = resident_range(c, "f", 50, 51);
        if (r == BP_OK) r = resident_targets(c, "f");
        CHECK(r == BP_ERR_ARG);
        CHECK(same(c, was));                                                                            // nothing moved on any failure
        c.has_targ = true; was.has_targ = true;
        CHECK(resident_targets(c, "f") == BP_OK && same(c, was));
    }
    CHECK(BP_ERR_ARG != BP_ERR_STATE && BP_ERR_ARG != BP_OK && BP_ERR_STATE != BP_OK);
}

static void test_unpad_rows()
{
    const int n = 3, sL = 5, ldL = 64;
    std::vector<float> src((size_t)n * ldL, -777.0f), dst((size_t)n * sL + 1, 555.0f);                  // pad columns poisoned; one float of guard
    for (int j = 0; j < n; ++j) for (int d = 0; d < sL; ++d) src[(size_t)j * ldL + d] = (float)(10 * j + d);
    unpad_rows(dst.data(), sL, src.data(), ldL, n);
    for (int j = 0; j < n; ++j) for (int d = 0; d < sL; ++d) CHECK(dst[(size_t)j * sL + d] == (float)(10 * j + d));
    CHECK(dst[(size_t)n * sL] == 555.0f);
    unpad_rows(dst.data(), sL, src.data(), ldL, 0);                                                     // no rows: nothing is touched
    CHECK(dst[0] == 0.0f && dst[(size_t)n * sL] == 555.0f);
}

// Seven differences whose squares are exact in fp32 (4096^2 = 2^24, 1^2 = 1), so the sums below do not depend on whether the
// compiler contracts e * e into the addition.  In fp32, 2^24 + 1 rounds back to 2^24 (ties to even): with 4096 first, frame-major /
// bin-minor order gives exactly 2^24; with the six 1s first they add up to 6 and 6 + 2^24 is exact.
static void test_sq_err_sum_order()
{
    const int n = 2, sL = 4, ldL = 64;                            // 2 frames x 4 bins: seven differences and one of 0
    const float big = 4096.0f;
    const float first_big[8] = {big, 1, 1, 1, 1, 1, 1, 0}, last_big[8] = {1, 1, 1, 1, 1, 1, 0, big};
    const float want[2] = {16777216.0f, 16777222.0f};
    for (int which = 0; which < 2; ++which) {
        const float *diff = which ? last_big : first_big;
        std::vector<float> out((size_t)n * ldL, 1e30f);           // (pad columns poisoned: never read)
        std::vector<float> targ((size_t)n * sL);
        for (int j = 0; j < n; ++j)
            for (int d = 0; d < sL; ++d) { targ[(size_t)j * sL + d] = (float)(3 * j - d); out[(size_t)j * ldL + d] = targ[(size_t)j * sL + d] + diff[j * sL + d]; }
        // 1. contiguous caller rows (bp_cv_chunk)
        const float *tp = targ.data();
        const float a = sq_err_sum(out.data(), ldL, sL, n, [&](int j) { return tp + (size_t)j * sL; });
        // 2. rows found through a table of frames (bp_cv_chunk_windows): the frames lie in another order, with one between them
        std::vector<float> frames((size_t)3 * sL, -5.0f);
        const int targ_frame[2] = {2, 0};
        for (int j = 0; j < n; ++j) memcpy(frames.data() + (size_t)targ_frame[j] * sL, tp + (size_t)j * sL, sizeof(float) * sL);
        const float *fp = frames.data();
        const float b = sq_err_sum(out.data(), ldL, sL, n, [&](int j) { return fp + (size_t)targ_frame[j] * sL; });
        // 3. rows in a block of their own that was copied back from the device (bp_cv_mix)
        std::vector<float> tg(targ);
        const float c = sq_err_sum(out.data(), ldL, sL, n, [&](int j) { return tg.data() + (size_t)j * sL; });
        if (!(a == want[which] && b == want[which] && c == want[which])) FAIL("case %d: %.1f %.1f %.1f, by hand %.1f", which, a, b, c, want[which]);
    }
    CHECK(sq_err_sum((const float *)nullptr, ldL, sL, 0, [](int) { return (const float *)nullptr; }) == 0.0f);
    CHECK(16777216.0f + 1.0f == 16777216.0f && 6.0f + 16777216.0f == 16777222.0f);                      // the fp32 facts the cases rest on
}

int main()
{
    name(MAIN, "main"); name(COPY, "copy");
    test_handshake_order();
    test_interleaved_uploads_wait_on_their_own_retire();
    test_every_maker_goes_through_the_one_transition();
    test_preconditions();
    test_unpad_rows();
    test_sq_err_sum_order();
    CHECK(g_ev == 0 && g_blocks == 0);
    printf("chunk_driver: handshake order, transition, preconditions and the way out agree (%zu stream and event calls)\n", g_log.size());
    return 0;
}
