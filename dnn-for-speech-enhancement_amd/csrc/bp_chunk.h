// bp_chunk.h -- the resident chunk of a handle: ONE record (Resident, bp_handle::res), one way in (make_resident; refill_begin /
// refill_end around the copies of an upload), one set of preconditions for the calls that read it (resident_range,
// resident_targets) and the host side of the way out (unpad_rows, sq_err_sum).  Internal: nothing in here is part of the C ABI.
// Like bp_mem.h this header names the HIP runtime's calls but includes no HIP header: the units include <hip/hip_runtime.h> first,
// the test program (tests/cpp/chunk_driver.cc) stands logging functions in for them.  What launches or allocates is bp_step.hip's.
//
// The invariants, held by the functions below and by nobody else:
//   - frames / windows / has_targ are written by make_resident alone, which also bumps gen, voids pre and resets next_first: a tile
//     pre-staged from the chunk before is never trained on, whoever made the new chunk resident.
//   - A STACKED chunk (bp_upload_chunk: the caller hands [frames][layersizes[0]] rows, the reference's interface, BP_GPU.cu:127-130)
//     lies in pair[cur]; a WINDOW chunk (bp_upload_chunk_windows: raw frames + index tables) stays as it is uploaded,
//     in wset[wcur] under the views wv, and every bunch stacks ITS rows into a staged tile right before its forward.  An upload fills
//     the copy that is not current; that copy's Retire says when the main stream has finished reading it.  The two kinds retire
//     apart: a stacked upload never waits for window work, nor a window upload for stacked work.
//   - has_targ is the ONE fact "the call that made the chunk resident supplied targets" (stacked: pair[cur].targ was written;
//     window: wv.tg != null); training and gradient calls need it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "bp_mem.h"

struct Retire { Event ev; bool valid; };   // main stream: the copy that is NOT current is no longer read (valid: recorded at least once)
struct WinSet { Buf r[4]; };               // raw frames, raw target frames, NAT rows, tables (win_start | targ_frame | nat_row)

struct Resident {
    int frames; bool windows, has_targ;       // rows of the resident chunk; it is a window chunk; it came with targets
    unsigned gen;                             // bumped by every chunk that becomes resident
    struct Pair { float *in, *targ; } pair[2];   // stacked: [cap + 64][ld_0], [cap + 64][ld_L], each pair allocated on its first use
    int cur; Retire retired;
    WinSet wset[2]; int wcur; Retire wretired;   // window: two grow-only staging sets
    struct { const float *fea, *tg, *nat; const int *ws, *tf, *nr; int D, win; } wv;   // views of set wcur
    // two staged tiles [Bp][ld_0], [Bp][ld_L]: while bunch i trains out of tile stage_cur, the output layer's reduce launch of bunch i
    // stacks bunch i+1 into the other (bp_out_split_stage)
    float *x0s2[2], *tgs2[2]; int stage_cur;
    int next_first;                           // chunk frame of the bunch that follows the one being enqueued (-1: none)
    struct { bool valid; int first, tile; uint32_t step; unsigned gen; } pre;   // what the other tile holds
    Event ev_copy;                            // copy stream: this chunk's H2D copies are done
    float *in() const { return pair[cur].in; }
    float *targ() const { return pair[cur].targ; }
    float *x0s() const { return x0s2[stage_cur]; }   // the staged bunch
    float *tgs() const { return tgs2[stage_cur]; }
};

// ------------------------------------------------------------------ the way in
static inline void make_resident(Resident &c, bool windows, int rows, bool has_targ)
{
    c.windows = windows; c.frames = rows; c.has_targ = has_targ;
    c.gen++; c.pre.valid = false; c.next_first = -1;    // (a tile pre-staged from the old chunk is void)
}
// Everything queued on `main` so far read the copy that was current: record that, and the other copy is the current one.
static inline int retire_and_flip(Retire &r, int &cur, hipStream_t main)
{
    HIPCHK(hipEventRecord(r.ev, main));
    r.valid = true; cur = 1 - cur;
    return BP_OK;
}
// An upload into the copy that is not current: refill_begin, the copies on the copy stream -- the bunches of the previous chunk,
// still running on the main stream out of the current copy, overlap them --, refill_end.  The caller may overwrite its buffers as
// soon as refill_end returns (BPtrain.cc:50-53).
static inline int refill_begin(const Retire &r, hipStream_t copy)
{
    if (r.valid) HIPCHK(hipStreamWaitEvent(copy, r.ev, 0));
    return BP_OK;
}
static inline int refill_end(Resident &c, Retire &r, int &cur, hipStream_t copy, hipStream_t main)
{
    HIPCHK(hipEventRecord(c.ev_copy, copy));
    HIPCHK(hipStreamSynchronize(copy));
    HIPCHK(hipStreamWaitEvent(main, c.ev_copy, 0));
    return retire_and_flip(r, cur, main);
}

// ------------------------------------------------------------------ preconditions of the calls that read the resident chunk
static inline int resident_range(const Resident &c, const char *who, long first, long n, const char *what = "frame range")
{
    if (first >= 0 && n >= 0 && first + n <= c.frames) return BP_OK;
    return fail(BP_ERR_ARG, std::string(who) + ": " + what + " outside the resident chunk");
}
static inline int resident_targets(const Resident &c, const char *who)
{
    if (c.has_targ) return BP_OK;
    return fail(BP_ERR_STATE, std::string(who) + ": the resident " + (c.windows ? "window" : "stacked") + " chunk was uploaded without targets (forward / CV upload)");
}

// ------------------------------------------------------------------ the way out, host side
// n rows of sL floats out of padded rows of ldL
static inline void unpad_rows(float *dst, int sL, const float *src, int ldL, int n)
{
    for (int j = 0; j < n; ++j) memcpy(dst + (size_t)j * sL, src + (size_t)j * ldL, sizeof(float) * sL);
}
// The CV sum: fp32, frame-major / bin-minor (BP_GPU.cu:458-467).  targ_row(j): the sL targets of frame j.
template <class TargRow>
static inline float sq_err_sum(const float *host_out, int ldL, int sL, int n, TargRow targ_row)
{
    float squared_err = 0.0f;
    for (int j = 0; j < n; ++j) {
        const float *t = targ_row(j);
        for (int d = 0; d < sL; ++d) { const float e = host_out[(size_t)j * ldL + d] - t[d]; squared_err = squared_err + e * e; }
    }
    return squared_err;
}
