// stream_core_driver.cc -- the host part of csrc/bp_stream_core.h on its own (no HIP, no library): the counts against the two
// formulas they replaced, and every push of a set of schedules through the carry, in both parameterisations -- the net's
// (look-ahead la, 6 warm-up frames with a noise-aware row) and log-MMSE's (no look-ahead, init_frames warm-up frames).  Built with
// -fsanitize=address,undefined: the carry's buffer, the segment and each push's samples are heap blocks of their exact sizes, so
// an access past any of them ends the run.  Exits non-zero with a message on the first mismatch.
#include <stdio.h>
#include <stdlib.h>

#include "bp_stream_core.h"

#define FAIL(...) do { printf("stream_core_driver: " __VA_ARGS__); printf("\n"); exit(1); } while (0)

// the formulas of bp_stream.hip and bp_classic.hip before they shared one
static Counts old_net_counts(int hop, int la, bool nat, int64_t received, bool ended)
{
    Counts c = {0, 0, 0};
    if (received <= 0) return c;
    const int64_t T = (received - 1) / hop + 2;
    c.fi = ended ? T : received / hop;
    const bool known = !nat || ended || c.fi >= 6;
    c.fo = !known ? 0 : ended ? T : std::max<int64_t>(0, c.fi - la);
    c.so = ended ? received : std::max<int64_t>(0, c.fo - 1) * hop;
    return c;
}
static Counts old_lm_counts(int hop, int init_frames, int64_t received, bool ended)
{
    Counts c = {0, 0, 0};
    if (received <= 0) return c;
    const int64_t T = (received - 1) / hop + 2;
    c.fi = ended ? T : received / hop;
    const bool known = ended || c.fi >= init_frames;
    c.fo = !known ? 0 : c.fi;
    c.so = ended ? received : std::max<int64_t>(0, c.fo - 1) * hop;
    return c;
}
static bool same(const Counts &a, const Counts &b) { return a.fi == b.fi && a.fo == b.fo && a.so == b.so; }

struct Mode { bool lm; int la, warm; };               // lm: frames are laid out when they get output (fo), else when analysed (fi)
struct Push { int n; bool end; };

// the pushes that deliver a sentence of L samples
static std::vector<Push> schedule(int kind, int L, int hop)
{
    std::vector<Push> v;
    const int ragged[3] = {17, 18, 19};
    switch (kind) {
    case 0: v.push_back({L, true}); break;                                                    // everything in one push
    case 1: for (int at = 0; at < L; at += hop) v.push_back({std::min(hop, L - at), at + hop >= L}); break;
    case 2: for (int at = 0; at < L; ++at) v.push_back({1, at + 1 == L}); break;
    case 3: for (int at = 0, k = 0; at < L; ++k) { const int n = std::min(ragged[k % 3], L - at); at += n; v.push_back({n, at == L}); } break;
    case 4: v.push_back({L / 2, false}); v.push_back({0, false}); v.push_back({L - L / 2, true}); break;   // a zero-length push in the middle
    default: v.push_back({L, false}); v.push_back({0, true}); break;                        // the end flag on an empty push after data
    }
    return v;
}

// Plays the sentences one after the other through one carry, as the push functions do, and checks every push.
static long play(const Mode &m, int hop, const std::vector<int> &lens, int kind)
{
    const size_t cap = m.lm ? (size_t)(m.warm + 2) * hop : (size_t)2 * hop;
    Carry carry(cap, hop);
    long pushes = 0;
    for (size_t si = 0; si < lens.size(); ++si) {
        const int L = lens[si];
        std::vector<float> P((size_t)hop, 0.0f);                                                // [hop zeros | sentence | zeros]
        for (int i = 0; i < L; ++i) P.push_back((float)(1 + i + 1000 * (int)si));
        P.resize(P.size() + (size_t)3 * hop, 0.0f);
        int at = 0;
        for (const Push &pu : schedule(kind, L, hop)) {
            ++pushes;
            if (carry.received != at) FAIL("received is %lld after %d samples", (long long)carry.received, at);
            float *in = pu.n ? new float[pu.n] : nullptr;
            for (int i = 0; i < pu.n; ++i) in[i] = P[(size_t)hop + at + i];
            const ChanStep p = stream_step(hop, m.la, m.warm, carry.received, pu.n, pu.end);
            const int64_t f0 = m.lm ? p.c0.fo : p.c0.fi, f1 = m.lm ? p.c1.fo : p.c1.fi, nf = f1 - f0;
            if (p.r1 != at + pu.n || nf < 0) FAIL("plan: r1 %lld, %lld new frames", (long long)p.r1, (long long)nf);
            if (nf > 0) {                                                                       // frames f0 .. f1 - 1 of the padded sentence
                const size_t seg = (size_t)(nf + 1) * hop;
                float *x = new float[seg];
                for (size_t i = 0; i < seg; ++i) x[i] = -1.0f;
                carry.fill_segment(x, seg, in, (size_t)pu.n);
                for (size_t i = 0; i < seg; ++i)
                    if (x[i] != P[(size_t)f0 * hop + i])
                        FAIL("hop %d lm %d la %d warm %d kind %d len %d: segment sample %zu of frames %lld .. %lld is %g, the sentence has %g", hop, m.lm,
                             m.la, m.warm, kind, L, i, (long long)f0, (long long)f1, x[i], P[(size_t)f0 * hop + i]);
                delete[] x;
            }
            if (p.ended) {
                carry.reset(hop);
                if (carry.received != 0 || carry.n != (size_t)hop) FAIL("reset leaves received %lld, %zu samples", (long long)carry.received, carry.n);
                for (int i = 0; i < hop; ++i) if (carry.buf[i] != 0.0f) FAIL("reset leaves sample %d = %g", i, carry.buf[i]);
            } else if (pu.n > 0) {
                const size_t keep = m.lm ? (size_t)hop + (size_t)(p.r1 - p.c1.fo * hop) : (size_t)hop + (size_t)(p.r1 % hop);
                if (keep > cap) FAIL("hop %d lm %d warm %d len %d: keep %zu exceeds the capacity %zu", hop, m.lm, m.warm, L, keep, cap);
                if (!carry.keep_last(in, (size_t)pu.n, keep)) FAIL("keep_last refused %zu of %zu + %d samples", keep, carry.n, pu.n);
                if (carry.n != keep || carry.received != p.r1 || carry.buf.size() != cap) FAIL("keep_last: %zu samples held, keep is %zu", carry.n, keep);
                for (size_t i = 0; i < keep; ++i)                                               // the last keep samples of the padded sentence so far
                    if (carry.buf[i] != P[(size_t)hop + p.r1 - keep + i]) FAIL("hop %d kind %d len %d: carry sample %zu of %zu is wrong", hop, kind, L, i, keep);
            }
            at = p.ended ? 0 : (int)p.r1;
            delete[] in;
        }
        if (carry.received != 0 || carry.n != (size_t)hop) FAIL("the sentence of %d samples did not end", L);
    }
    return pushes;
}

int main()
{
    long checked = 0, pushes = 0;
    for (int hop : {32, 128}) {
        std::vector<Mode> modes;
        for (int la : {0, 3, 6}) for (int nat = 0; nat < 2; ++nat) {
            modes.push_back({false, la, nat ? 6 : 0});
            for (int e = 0; e < 2; ++e) for (int64_t r = 0; r <= (6 + 3) * hop + 1; ++r, ++checked)
                if (!same(stream_counts(hop, la, nat ? 6 : 0, r, e), old_net_counts(hop, la, nat, r, e))) FAIL("net counts differ: hop %d la %d nat %d r %lld e %d", hop, la, nat, (long long)r, e);
        }
        for (int init : {1, 4, 6}) {
            modes.push_back({true, 0, init});
            for (int e = 0; e < 2; ++e) for (int64_t r = 0; r <= (init + 3) * hop + 1; ++r, ++checked)
                if (!same(stream_counts(hop, 0, init, r, e), old_lm_counts(hop, init, r, e))) FAIL("log-MMSE counts differ: hop %d init %d r %lld e %d", hop, init, (long long)r, e);
        }
        const std::vector<int> lens = {1, hop - 1, hop, hop + 1, 5 * hop + 7};
        for (const Mode &m : modes)
            for (int kind = 0; kind < 6; ++kind)
                for (size_t i = 0; i < lens.size(); ++i) {
                    pushes += play(m, hop, {lens[i]}, kind);
                    pushes += play(m, hop, {lens[i], lens[(i + 1) % lens.size()]}, kind);           // two sentences back to back on one channel
                }
        // keep_last never writes past the capacity: more than the capacity, or more than there is, is refused and changes nothing
        Carry c((size_t)2 * hop, hop);
        std::vector<float> big((size_t)3 * hop, 1.0f);
        if (c.keep_last(big.data(), big.size(), (size_t)2 * hop + 1) || c.keep_last(big.data(), 1, (size_t)hop + 2) || c.n != (size_t)hop || c.received != 0)
            FAIL("keep_last accepted more than the capacity or more than there is");
        if (!c.keep_last(big.data(), big.size(), (size_t)2 * hop) || c.n != (size_t)2 * hop) FAIL("keep_last refused the capacity");
    }
    // the push checks: the messages with the caller's name
    const int n_in[3] = {4, -1, 9}, ok_in[3] = {4, 0, 9};
    const float x[13] = {0};
    int64_t total = -1;
    if (stream_push_checks("f", 3, 100, n_in, x, &total) != "f: n_in[1] < 0" || stream_push_checks("f", 3, 12, ok_in, x, &total) != "f: more than max_push_samples = 12 samples in one push" ||
        stream_push_checks("f", 3, 13, ok_in, nullptr, &total) != "f: null pcm" || total != -1 || !stream_push_checks("f", 3, 13, ok_in, x, &total).empty() || total != 13)
        FAIL("stream_push_checks");
    if (stream_out_checks("f", 5, 4, x) != "f: 5 samples are due, out_cap is 4" || stream_out_checks("f", 5, 5, nullptr) != "f: null out_pcm" ||
        !stream_out_checks("f", 0, 0, nullptr).empty() || !stream_out_checks("f", 5, 5, x).empty())
        FAIL("stream_out_checks");
    printf("stream_core_driver: %ld counts and %ld pushes agree\n", checked, pushes);
    return 0;
}
