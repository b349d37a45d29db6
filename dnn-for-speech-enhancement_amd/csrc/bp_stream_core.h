// bp_stream_core.h -- what the two streaming engines share (bp_stream.hip: the net; bp_classic.hip: log-MMSE): what a channel has
// produced after `received` samples, its carry, the checks of a push, and the owner of a stream's device and pinned blocks.
// Internal: nothing in here is part of the C ABI.  The host part (everything above the __HIP__ guard) needs no HIP header and is
// tested on its own (tests/cpp/stream_core_driver.cc).
//
// A sentence is padded with hop zeros in front and zeros behind; frame t covers the padded samples [t hop, (t + 2) hop).  The
// engines differ in what a frame waits for, not in the framing.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace {

// What a channel has produced after `received` samples of its sentence (include/bp_c_api.h: bp_stream_counts,
// bp_lmstream_counts): frames analysed fi, frames enhanced fo, samples returned so.  No frame is enhanced before warmup_frames
// are analysed (or the sentence has ended); from then on a frame waits for look_ahead frames behind it.
struct Counts { int64_t fi, fo, so; };
inline Counts stream_counts(int hop, int look_ahead, int warmup_frames, int64_t received, bool ended)
{
    Counts c = {0, 0, 0};
    if (received <= 0) return c;
    const int64_t T = (received - 1) / hop + 2;
    c.fi = ended ? T : received / hop;
    const bool known = ended || c.fi >= warmup_frames;
    c.fo = !known ? 0 : ended ? T : std::max<int64_t>(0, c.fi - look_ahead);
    c.so = ended ? received : std::max<int64_t>(0, c.fo - 1) * hop;
    return c;
}

// One channel's part of one push: the counts before and after it.  Planned from the numbers alone, before anything changes.
struct ChanStep { int64_t r1; bool ended; Counts c0, c1; };
inline ChanStep stream_step(int hop, int look_ahead, int warmup_frames, int64_t received, int n_in, bool end_flag)
{
    ChanStep p;
    p.r1 = received + n_in;
    p.ended = end_flag && p.r1 > 0;
    p.c0 = stream_counts(hop, look_ahead, warmup_frames, received, false);
    p.c1 = stream_counts(hop, look_ahead, warmup_frames, p.r1, p.ended);
    return p;
}

// A channel's sentence so far: the samples received and the carry, the padded samples from the start of its next new frame on
// (hop zeros in front of a sentence).  The capacity is fixed at construction and no operation writes past it.
struct Carry {
    int64_t received;            // samples of the current sentence
    size_t n;                    // samples held
    std::vector<float> buf;
    Carry(size_t capacity, size_t hop) : received(0), n(hop), buf(capacity, 0.0f) {}
    void reset(size_t hop) { received = 0; n = hop; memset(buf.data(), 0, hop * sizeof(float)); }   // a new sentence
    // dst[0 .. seg) = [carry | new | zeros] (zeros: behind a sentence's end); what does not fit seg is left out
    void fill_segment(float *dst, size_t seg, const float *in, size_t n_in) const
    {
        const size_t nca = std::min(seg, n), nin = std::min(seg - nca, n_in);
        memcpy(dst, buf.data(), nca * sizeof(float));
        if (nin) memcpy(dst + nca, in, nin * sizeof(float));
        memset(dst + nca + nin, 0, (seg - nca - nin) * sizeof(float));
    }
    // n_in samples were received: the carry becomes the last `keep` samples of [carry | new]; false (and nothing changed) if that
    // is more than the capacity or more than there is
    bool keep_last(const float *in, size_t n_in, size_t keep)
    {
        if (keep > buf.size() || keep > n + n_in) return false;
        if (n_in >= keep) memcpy(buf.data(), in + (n_in - keep), keep * sizeof(float));
        else {
            const size_t old = keep - n_in;                          // (old <= n: checked above)
            memmove(buf.data(), buf.data() + (n - old), old * sizeof(float));
            memcpy(buf.data() + old, in, n_in * sizeof(float));
        }
        n = keep; received += (int64_t)n_in;
        return true;
    }
};

// The checks at the top of a push, before the plan; the message of the first that fails, or none.
inline std::string stream_push_checks(const char *who, int n_chan, int max_push, const int *n_in, const float *pcm, int64_t *total_in)
{
    const std::string w(who);
    int64_t total = 0;
    for (int c = 0; c < n_chan; ++c) {
        if (n_in[c] < 0) return w + ": n_in[" + std::to_string(c) + "] < 0";
        total += n_in[c];
        if (total > max_push) return w + ": more than max_push_samples = " + std::to_string(max_push) + " samples in one push";
    }
    if (total > 0 && !pcm) return w + ": null pcm";
    *total_in = total;
    return std::string();
}
// ... and behind it, once the samples due are known
inline std::string stream_out_checks(const char *who, int64_t due, size_t out_cap, const float *out_pcm)
{
    if ((size_t)due > out_cap) return std::string(who) + ": " + std::to_string(due) + " samples are due, out_cap is " + std::to_string(out_cap);
    if (due > 0 && !out_pcm) return std::string(who) + ": null out_pcm";
    return std::string();
}

}  // namespace

#ifdef __HIP__
#include <hip/hip_runtime.h>

#include "bp_mem.h"

// The blocks of a stream: one device block (constants | state | a push's input block | its output samples, laid out by the
// engine) and the pinned host ends of the two copies of a push, freed with the stream.
struct StreamBlocks {
    Buf dev, pin_in, pin_out;
    hipError_t alloc(size_t dev_bytes, size_t pin_in_bytes, size_t pin_out_bytes)
    {
        hipError_t e = dev.alloc(dev_bytes);
        if (e == hipSuccess) e = pin_in.alloc(pin_in_bytes, true);
        if (e == hipSuccess) e = pin_out.alloc(pin_out_bytes, true);
        return e;
    }
    // at open: the constants the engine wrote to pin_in[0 .. consts) go to the front of the device block, the state behind
    // them, [consts, state_end), starts as zeros
    hipError_t upload_consts(size_t consts, size_t state_end, hipStream_t st)
    {
        hipError_t e = hipMemcpyAsync(dev.p, pin_in.p, consts, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(dev.as<char>() + consts, 0, state_end - consts, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        return e;
    }
    // the end of a push: the `due` samples at dev + o_out come back, the one synchronisation, and they go to the caller
    hipError_t copy_back(size_t o_out, int64_t due, float *out_pcm, hipStream_t st)
    {
        hipError_t e = due > 0 ? hipMemcpyAsync(pin_out.p, dev.as<char>() + o_out, (size_t)due * 4, hipMemcpyDeviceToHost, st) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess && due > 0) memcpy(out_pcm, pin_out.p, (size_t)due * 4);
        return e;
    }
};
#endif
