// bp_stream.hip -- C-ABI implementation (include/bp_c_api.h): streaming sessions.  Audio that is still arriving is
// enhanced in blocks of any sizes, on n_chan independent channels per push, and returns the SAME BITS as one bp_enhance_waves
// call on the finished sentence: the analysis and the synthesis are the device functions of bp_wave.hip (bp_fft.h), the forward
// is forward_resident on a window chunk, and the overlap-add is the same gather of two frames.  gfx950 only.
//
// What a channel has after `received` samples of its sentence is a pure function of that number (stream_counts in
// bp_stream_core.h, exported as bp_stream_counts): frames analysed fi, frames enhanced fo, samples returned.  The host plans a
// push from those numbers alone and never reads device state.  It keeps each channel's carry (bp_stream_core.h: here the last
// hop + received % hop samples) and builds ONE pinned input block per push: three job tables and every active channel's [carry | new] samples at hop-aligned places, so
// that the frame loads of the analysis are the aligned 16-byte loads of rfft_frame.
//
// Device state of a channel (allocated at open, R = context + 6 slots, all of it double-buffered by a parity that the host flips
// whenever a push touches it, so that no launch reads what another workgroup of the same launch writes):
//   rows  the normalised rows of frames [max(0, fo - targ_offset), fi): the history the next windows need
//   Y     the noisy spectra of frames [fo, fi): analysed, waiting for their look-ahead (same slots as the rows)
//   nat   the noise-aware row of the sentence (single: written once per sentence, by a launch of its own)
//   half  the second half of the last synthesised frame
//
// Kernels (one workgroup of 256 threads per job; tables in the input block):
//   bp_stream_analysis   a new frame: window, FFT, Y, LPS, normalised row -- or an old frame: its row (and Y) from the state.  Either
//                        goes where it is needed: the staged rows of the push's window chunk (replicated at the sentence's edges),
//                        the Y of the push, the other parity of the state; plus the frame's win_start / nat_row entries
//   bp_stream_nat        the noise-aware row, once per sentence, in bp_wave_nat's summation order; later pushes copy it into the chunk
//   bp_stream_dnat       a stream opened in BP_NAT_DYNAMIC (bp_set_nat) instead: one noise-aware row per enhanced frame, from the push's Y
//                        (and for a sentence's noise start the Y that still waits in the state); lambda and pbar [n_chan][D] carried
//   bp_stream_synthesis  per enhanced frame: its synthesis, the synthesis of the frame before it when that is of the same push
//                        (else the carried half), overlap-add into the compact output, the new carried half
//
// Where a frame sits in its bunch matters: the forward kernels give a row the same bits whoever its neighbours are, but NOT at
// every row of the bunch (the in-workgroup k-split of the narrow-layer GEMM hands rows 16..23 and 24..31 of a tile to waves that add
// the four partial sums in another order; measured: one sentence alone and the same sentence behind others differ in the last bit).
// bp_enhance_waves on one sentence runs frame t as row t mod bunchsize, so a push places frame t of a channel at a sample g with
// g = t (mod bunchsize): the channels of a push start in bunches of their own unless their rows happen to follow each other, and
// the samples in between are fillers (window 0, computed and ignored).
// A stream opened while the handle is in BP_FORWARD_ROWINV (bp_set_forward) runs the row-invariant forward of bp_infer.hip, whose
// bits do not depend on the row: it is `packed` -- the frames of a push follow each other in channel order, without fillers, and a
// push of n frames costs ceil(n / bunchsize) bunches whatever the number of channels.  The mode is the stream's from then on.
// No float atomics.  Per push: one host->device copy, one device->host copy, one synchronisation.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "bp_classic.h"
#include "bp_fft.h"
#include "bp_handle.h"
#include "bp_stream_core.h"

namespace {

// src >= 0: analyse the frame at hop unit src of the block's samples; src < 0: copy state slot -1 - src.
// Staged rows [stage_lo, stage_hi) of the window chunk get the row; state_dst (or -1) is its slot in the new parity;
// g >= 0: the frame is enhanced by this push as sample g of the window chunk (win_start[g] = ws, nat_row[g] = chan) and its Y
// goes to row y of the push's Y; y_state >= 0: the frame waits, Y to that slot.  has_y: a copied frame whose Y is still needed.
struct AnaJob { int src, stage_lo, stage_hi, state_dst, g, ws, chan, y_state, has_y, y, pad[2]; };
// mode 0: from the staged rows (src = row of frame 0), 1: from the state rows (src = slot of frame 0), 2: copy the state's row.
// nf = min(T, 6) frames exist; stage: also into the chunk's NAT rows.
struct NatJob { int chan, mode, src, nf, stage, pad[3]; };
// A stream in BP_NAT_DYNAMIC (bp_set_nat) has these in place of NatJobs, one per channel that gets frames enhanced in a push: frames
// t0 .. t0 + ne - 1 of the channel's sentence, frame t0 + i being row y + i of the push's Y and noise-aware row g + i of the chunk.
// t0 == 0: the job starts the sentence -- the noise start is over its first ni = min(6, T) frames, frame t of them in row y + t of
// the push's Y while t < ne and, still waiting for its look-ahead, in slot st + t - ne of the state's NEW parity beyond.
// ended: the sentence is over and nothing is carried.
struct DnatJob { int chan, t0, ne, y, g, ni, st, ended; };
static_assert(sizeof(DnatJob) == sizeof(NatJob), "the two job tables share their place in the input block");
// The frame is sample g of the chunk (its net output) and row y of the push's Y.  prev: -1 none (frame 0 of a sentence: front
// padding, no output), 0 the frame before it is of this push too (sample g - 1, row y - 1), 1 the carried half in slot half_src.
// out_n samples to out_off of the compact output; half_dst (or -1): where the second half goes.
struct SynJob { int g, prev, half_src, out_off, out_n, half_dst, y, pad; };

struct StreamAnaArgs {
    const AnaJob *jobs; const float *pcm, *win; const float2 *tw; const float *mean, *inv_std;
    int log2M, D, hop;
    float *st_rows; float2 *st_Y;       // [2][n_chan][R][D]
    float *rows; float2 *Y;             // the push: staged rows of the window chunk, Y[y][D]
    int *win_start, *nat_row;
    int nat_frame;                      // nat_row[g] = the channel (0) or g itself (1: bp_stream_dnat writes one row per sample)
};

}  // namespace

__global__ __launch_bounds__(WAVE_THREADS) void bp_stream_analysis(const StreamAnaArgs a)
{
    extern __shared__ float2 z[];
    const AnaJob j = a.jobs[blockIdx.x];
    const int M = 1 << a.log2M, tid = threadIdx.x;
    if (j.src >= 0) rfft_frame(z, a.pcm + (size_t)j.src * a.hop, a.win, a.tw, a.log2M);
    for (int k = tid; k <= M; k += blockDim.x) {
        float v;
        float2 X = make_float2(0.0f, 0.0f);
        if (j.src >= 0) {
            X = rfft_bin(z, a.tw, M, k);
            const float p = X.x * X.x + X.y * X.y;
            const float l = lps_of(p);
            v = (l - a.mean[k]) * a.inv_std[k];
        } else {
            const size_t si = (size_t)(-1 - j.src) * a.D + k;
            v = a.st_rows[si];
            if (j.has_y) X = a.st_Y[si];
        }
        for (int u = j.stage_lo; u < j.stage_hi; ++u) a.rows[(size_t)u * a.D + k] = v;
        if (j.state_dst >= 0) a.st_rows[(size_t)j.state_dst * a.D + k] = v;
        if (j.g >= 0) a.Y[(size_t)j.y * a.D + k] = X;
        if (j.y_state >= 0) a.st_Y[(size_t)j.y_state * a.D + k] = X;
    }
    if (j.g >= 0 && tid == 0) { a.win_start[j.g] = j.ws; if (a.nat_row) a.nat_row[j.g] = a.nat_frame ? j.g : j.chan; }
}

// nat[k] = ((((v0 + v1) + v2) + v3) + v4 + v5) / 6 over the sentence's first 6 normalised frames, frame f clamped to nf - 1
__global__ __launch_bounds__(WAVE_THREADS) void bp_stream_nat(const NatJob *__restrict__ jobs, const float *__restrict__ rows,
                                                           const float *__restrict__ st_rows, int D, float *__restrict__ st_nat,
                                                           float *__restrict__ nat)
{
    const int kb = (D + WAVE_THREADS - 1) / WAVE_THREADS, k = (blockIdx.x % kb) * WAVE_THREADS + threadIdx.x;
    const NatJob j = jobs[blockIdx.x / kb];
    if (k >= D) return;
    float out;
    if (j.mode == 2) out = st_nat[(size_t)j.chan * D + k];
    else {
        const float *r = (j.mode == 0 ? rows : st_rows) + (size_t)j.src * D + k;
        float acc = 0.0f;
        for (int f = 0; f < 6; ++f) { const float v = r[(size_t)(f < j.nf ? f : j.nf - 1) * D]; acc = f == 0 ? v : acc + v; }
        out = acc / 6.0f;
        st_nat[(size_t)j.chan * D + k] = out;
    }
    if (j.stage) nat[(size_t)j.chan * D + k] = out;
}

namespace {
constexpr int DNAT_THREADS = 64;
struct StreamDnatArgs {
    const DnatJob *jobs; const float2 *Y, *st_Y; const float *mean, *inv_std;
    double *lam, *pb;                   // [n_chan][D]: the tracker's state between pushes
    float *nat;                         // the chunk's noise-aware rows, one per sample
    int D; NoiseP np;
};
}  // namespace

// The dynamic noise-aware rows of a push: one thread per (job, bin), serial over the job's frames, the step
// lm_dnat of bp_wave_dnat (bp_classic.h) and its noise start (lm_power in ascending t from 0.0, lm_noise_start): the rows of
// bp_enhance_waves in the same mode whatever the block sizes.  lambda and pbar wait in the channel's state between pushes; a
// thread reads and writes its own two doubles only.  No LDS, no barrier.
__global__ __launch_bounds__(DNAT_THREADS) void bp_stream_dnat(const StreamDnatArgs a)
{
#pragma clang fp contract(off)
    const int D = a.D, kb = (D + DNAT_THREADS - 1) / DNAT_THREADS, k = (blockIdx.x % kb) * DNAT_THREADS + threadIdx.x;
    const DnatJob j = a.jobs[blockIdx.x / kb];
    if (k >= D) return;
    const float2 *Y = a.Y + (size_t)j.y * D + k;
    double lam = 0.0, pb = 0.0;
    if (j.t0 == 0) {
        for (int t = 0; t < j.ni; ++t) lam += lm_power(t < j.ne ? Y[(size_t)t * D] : a.st_Y[(size_t)(j.st + t - j.ne) * D + k]);
        lam = lm_noise_start(lam, j.ni);
    } else { lam = a.lam[(size_t)j.chan * D + k]; pb = a.pb[(size_t)j.chan * D + k]; }
    const float mean = a.mean[k], istd = a.inv_std[k];
    float *nat = a.nat + (size_t)j.g * D + k;
    float2 cur = Y[0];
    for (int i = 0; i < j.ne; ++i) {
        const float2 nxt = Y[(size_t)(i + 1 < j.ne ? i + 1 : i) * D];   // (in flight under the chain of frame i)
        nat[(size_t)i * D] = lm_dnat(a.np, cur, lam, pb, mean, istd);
        cur = nxt;
    }
    if (!j.ended) { a.lam[(size_t)j.chan * D + k] = lam; a.pb[(size_t)j.chan * D + k] = pb; }
}

namespace {
// floats of LDS in front of the two frames of bp_stream_synthesis: synth_frame's FFT space and S, rounded up to 16 bytes
__host__ __device__ inline size_t syn_frames_at(int M) { return ((lds_bytes(M) + (size_t)(M + 1) * sizeof(float2) + 15) & ~(size_t)15) / sizeof(float); }
struct StreamSynArgs {
    const SynJob *jobs;
    const float *out; int ldo, out_col;     // net outputs [n][ldo], columns [out_col, out_col + D)
    const float2 *Y; const float *win; const float2 *tw;
    int log2M, D, target;
    float *half;                            // [2][n_chan][hop]
    float *pcm;                             // compact output of the push
};
}  // namespace

// (Post: NoPost, or PostFn for a stream opened with post-processing on, bp_set_post)
template <class Post>
__global__ __launch_bounds__(WAVE_THREADS) void bp_stream_synthesis(const StreamSynArgs a, const Post post)
{
    extern __shared__ __align__(16) float2 zs[];
    float2 *z = zs;
    const SynJob j = a.jobs[blockIdx.x];
    const int M = 1 << a.log2M, N = 2 * M, hop = M;
    float *cur = reinterpret_cast<float *>(zs) + syn_frames_at(M), *prev = cur + N;   // two frames behind synth_frame's space
    synth_frame(z, a.out + (size_t)j.g * a.ldo + a.out_col, a.Y + (size_t)j.y * a.D, a.win, a.tw, a.log2M, a.target, cur, post);
    __syncthreads();
    if (j.prev == 0) {
        synth_frame(z, a.out + (size_t)(j.g - 1) * a.ldo + a.out_col, a.Y + (size_t)(j.y - 1) * a.D, a.win, a.tw, a.log2M, a.target, prev, post);
        __syncthreads();
    }
    if (j.prev >= 0) {
        const float *pv = j.prev == 0 ? prev + hop : a.half + (size_t)j.half_src * hop;
        overlap_store(cur, pv, a.win, hop, a.pcm + j.out_off, j.out_n, blockDim.x);
    }
    if (j.half_dst >= 0) copy_half(a.half + (size_t)j.half_dst * hop, cur + hop, hop, blockDim.x);
}

// ------------------------------------------------------------------ host side
namespace {

struct Chan {
    int par, hpar;               // parity of the rows / Y state and of the carried half frame
    Carry carry;                 // [2 hop]: the samples the next frame starts with, hop + received % hop of them
};

// plan of one channel for one push
struct ChanPlan : ChanStep { int64_t g0; };   // g0: the chunk sample of the channel's first frame

}  // namespace

struct bp_stream {
    bp_handle *h;
    int D, ctx, toff, la, target, out_col, n_chan, max_push, hop, log2M, R;
    int warm;                    // frames before the first is enhanced: 6 with a noise-aware row (nat), else 0
    bool nat;
    bool dyn; NoiseP nat_np;     // opened in BP_NAT_DYNAMIC (bp_set_nat): one tracked noise-aware row per frame, with these parameters
    bool packed;                 // opened in BP_FORWARD_ROWINV: dense placement, the row-invariant forward on every push
    bool post; PostP pp;         // opened with post-processing on (bp_set_post): its parameters, centre and scale in a part of the stream's block
    std::vector<Chan> ch;
    std::vector<ChanPlan> plan;
    std::vector<AnaJob> ana; std::vector<NatJob> natj; std::vector<DnatJob> dnatj; std::vector<SynJob> syn;
    size_t max_enh;              // samples (frames to enhance) of one push at most
    StreamBlocks blk;            // device: consts | state | input block | Y of the push | output samples
    size_t o_mean, o_istd, o_win, o_tw, o_post, o_rows, o_Y, o_nat, o_half, o_lam, o_pb, o_in, o_pY, o_out, in_cap;
};

void stream_free_all(bp_handle *h)
{
    for (bp_stream *s : h->streams) delete s;
    h->streams.clear();
}

static int stream_cfg_check(const char *who, int fea_dim, int ctx, int toff)
{
    if (wave_log2_fft(fea_dim) < 0) return fail(BP_ERR_ARG, std::string(who) + ": 2*(fea_dim-1) must be a power of two from 64 to 2048");
    if (ctx < 1 || toff < 0 || toff >= ctx) return fail(BP_ERR_ARG, std::string(who) + ": need context >= 1 and 0 <= targ_offset < context");
    return BP_OK;
}

extern "C" int bp_stream_counts(int fea_dim, int context, int targ_offset, int nat, int64_t received, int ended, int64_t *frames_in,
                                int64_t *frames_out, int64_t *samples_out)
{
    { const int r = stream_cfg_check("bp_stream_counts", fea_dim, context, targ_offset); if (r != BP_OK) return r; }
    if (received < 0) return fail(BP_ERR_ARG, "bp_stream_counts: received < 0");
    if (!frames_in || !frames_out || !samples_out) return fail(BP_ERR_ARG, "bp_stream_counts: null output");
    const Counts c = stream_counts(fea_dim - 1, context - 1 - targ_offset, nat ? 6 : 0, received, ended != 0);
    *frames_in = c.fi; *frames_out = c.fo; *samples_out = c.so;
    return BP_OK;
}

extern "C" int bp_stream_open(bp_handle *h, const bp_stream_config *c, bp_stream **out)
{
    if (!h || !c || !out) return fail(BP_ERR_ARG, "bp_stream_open: null argument");
    { const int r = stream_cfg_check("bp_stream_open", c->fea_dim, c->context, c->targ_offset); if (r != BP_OK) return r; }
    const int D = c->fea_dim, ctx = c->context, L = h->L, sL = h->s[L - 1];
    if (!c->mean || !c->inv_std) return fail(BP_ERR_ARG, "bp_stream_open: null pointer");
    const bool nat = (long)h->s[0] == (long)(ctx + 1) * D;
    if (!nat && (long)h->s[0] != (long)ctx * D)
        return fail(BP_ERR_ARG, "bp_stream_open: layersizes[0] must be context*fea_dim or (context+1)*fea_dim");
    bool dyn;
    { const int r = wave_nat_mode("bp_stream_open", h, nat, &dyn); if (r != BP_OK) return r; }
    if (c->target != BP_WAVE_LPS && c->target != BP_WAVE_MASK) return fail(BP_ERR_ARG, "bp_stream_open: target must be BP_WAVE_LPS or BP_WAVE_MASK");
    if (c->out_col < 0 || (long)c->out_col + D > sL) return fail(BP_ERR_ARG, "bp_stream_open: out_col + fea_dim exceeds layersizes[last]");
    { const int r = wave_post_check("bp_stream_open", h, D, c->target); if (r != BP_OK) return r; }
    if (c->n_chan < 1 || c->n_chan > (1 << 16)) return fail(BP_ERR_ARG, "bp_stream_open: n_chan must be in 1 .. 65536");
    if (c->max_push_samples < 1) return fail(BP_ERR_ARG, "bp_stream_open: max_push_samples must be >= 1");
    if (h->dp) return fail(BP_ERR_STATE, "bp_stream_open: not on an attached data-parallel handle");
    HIPCHK(hipSetDevice(h->cfg.device));

    bp_stream *s = new bp_stream();
    s->h = h; s->D = D; s->ctx = ctx; s->toff = c->targ_offset; s->la = ctx - 1 - c->targ_offset; s->target = c->target;
    s->out_col = c->out_col; s->n_chan = c->n_chan; s->max_push = c->max_push_samples; s->hop = D - 1; s->log2M = wave_log2_fft(D);
    s->R = ctx + 6; s->nat = nat; s->warm = nat ? 6 : 0; s->packed = h->fwd_mode == BP_FORWARD_ROWINV;
    s->dyn = dyn; s->nat_np = h->nat_np;                         // the stream's from now on, as the forward's mode is
    s->post = h->post_on; s->pp = h->post;                       // ... and so is the post-processing (the arrays: copied below)
    const int hop = s->hop, N = 2 * hop, nc = s->n_chan;
    // A push analyses at most n_in/hop + 3 frames per channel (the end of a sentence adds up to 3) and enhances those plus the
    // frames that waited; it can never enhance more than the chunk capacity lets it stage.
    const size_t new_frames = (size_t)s->max_push / hop + 3 * (size_t)nc;
    const size_t max_ana = new_frames + (size_t)nc * s->R;
    s->max_enh = std::min(max_ana, (size_t)h->cap);
    Layout in;                                                   // the largest input block of a push (laid out by the push)
    in.take(max_ana * sizeof(AnaJob)); in.take((size_t)nc * sizeof(NatJob)); in.take(s->max_enh * sizeof(SynJob));
    in.take((new_frames + nc) * hop * 4);
    s->in_cap = in.size();
    const size_t slots = 2 * (size_t)nc * s->R;
    Layout lay;
    s->o_mean = lay.take((size_t)D * 4);
    s->o_istd = lay.take((size_t)D * 4);
    s->o_win = lay.take((size_t)N * 4);
    s->o_tw = lay.take((size_t)(hop + 1) * 8);
    s->o_post = lay.take(s->post ? 2 * (size_t)D * 4 : 0);      // centre | scale
    s->o_rows = lay.take(slots * D * 4);
    s->o_Y = lay.take(slots * D * 8);
    s->o_nat = lay.take((size_t)nc * D * 4);
    s->o_half = lay.take(2 * (size_t)nc * hop * 4);
    s->o_lam = lay.take(dyn ? (size_t)nc * D * 8 : 0); s->o_pb = lay.take(dyn ? (size_t)nc * D * 8 : 0);
    const size_t consts = s->o_rows;
    s->o_in = lay.take(s->in_cap);
    s->o_pY = lay.take(s->max_enh * D * 8);
    s->o_out = lay.take(s->max_enh * hop * 4);
    hipError_t e = s->blk.alloc(lay.size(), std::max(s->in_cap, consts), al256(s->max_enh * hop * 4));
    if (e != hipSuccess) { delete s; return fail(BP_ERR_NOMEM, std::string("bp_stream_open: ") + hipGetErrorString(e)); }
    int r = out_chunk_reserve(h, (int)(s->max_enh + (size_t)nc * h->B));   // (fillers included: so that no push has to grow it)
    if (r != BP_OK) { delete s; return r; }
    // constants, once: the norm file, window and twiddles (computed in double and rounded once, as bp_enhance_waves does)
    char *pin = s->blk.pin_in.as<char>();
    memset(pin, 0, consts);
    memcpy(pin + s->o_mean, c->mean, (size_t)D * 4);
    memcpy(pin + s->o_istd, c->inv_std, (size_t)D * 4);
    wave_window_twiddles(s->log2M, (float *)(pin + s->o_win), (float2 *)(pin + s->o_tw));
    if (s->post) { s->pp.c = (const float *)(s->blk.dev.as<char>() + s->o_post); s->pp.s = s->pp.c + D; }
    e = s->blk.upload_consts(consts, s->o_in, h->stream);
    if (e == hipSuccess && s->post && s->pp.gv) {                // centre and scale: device to device, from the handle's block
        e = hipMemcpyAsync((void *)s->pp.c, h->post.c, (size_t)D * 4, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync((void *)s->pp.s, h->post.s, (size_t)D * 4, hipMemcpyDeviceToDevice, h->stream);
    }
    if (e != hipSuccess) { delete s; return fail(BP_ERR_DEVICE, std::string("bp_stream_open: ") + hipGetErrorString(e)); }
    s->ch.assign(nc, Chan{0, 0, Carry((size_t)2 * hop, hop)});
    s->plan.resize(nc);
    s->ana.reserve(max_ana); s->natj.reserve(nc); s->dnatj.reserve(nc); s->syn.reserve(s->max_enh);
    h->streams.push_back(s);
    *out = s;
    return BP_OK;
}

extern "C" int bp_stream_packed(const bp_stream *s) { return s && s->packed ? 1 : 0; }

extern "C" int bp_stream_close(bp_stream *s)
{
    if (!s) return BP_OK;
    bp_handle *h = s->h;
    (void)hipSetDevice(h->cfg.device);
    (void)hipStreamSynchronize(h->stream);
    h->streams.erase(std::remove(h->streams.begin(), h->streams.end(), s), h->streams.end());
    delete s;
    return BP_OK;
}

extern "C" int bp_stream_push(bp_stream *s, const int *n_in, const float *pcm, const unsigned char *end, int *n_out, float *out_pcm,
                              size_t out_cap)
{
    if (!s || !n_in || !n_out) return fail(BP_ERR_ARG, "bp_stream_push: null argument");
    bp_handle *h = s->h;
    if (h->dp) return fail(BP_ERR_STATE, "bp_stream_push: not on an attached data-parallel handle");
    const int D = s->D, ctx = s->ctx, toff = s->toff, hop = s->hop, nc = s->n_chan, R = s->R, L = h->L, B = h->B;
    // ---- the plan: counts before and after, per channel (nothing of the stream changes until every check has passed)
    int64_t total_in = 0, due = 0, n = 0, n_enh = 0, rows = 0, ana_max = 0, active = 0;
    { const std::string m = stream_push_checks("bp_stream_push", nc, s->max_push, n_in, pcm, &total_in); if (!m.empty()) return fail(BP_ERR_ARG, m); }
    for (int c = 0; c < nc; ++c) {
        ChanPlan &p = s->plan[c];
        static_cast<ChanStep &>(p) = stream_step(hop, s->la, s->warm, s->ch[c].carry.received, n_in[c], end && end[c]);
        const int64_t ne = p.c1.fo - p.c0.fo;
        due += p.c1.so - p.c0.so; n_enh += ne;
        if (ne > 0) { p.g0 = s->packed ? n : n + ((p.c0.fo - n) % B + B) % B; n = p.g0 + ne; }      // frame t as row t mod B of its bunch; packed: any row
        if (ne > 0) rows += ne + ctx - 1;
        if (p.c1.fi > p.c0.fi) { ana_max += p.c1.fi - std::max<int64_t>(0, p.c0.fo - toff); ++active; }
        if (!p.ended && p.c1.fi - std::max<int64_t>(0, p.c1.fo - toff) > R)
            return fail(BP_ERR_STATE, "bp_stream_push: internal: channel state exceeds context + 6 frames");
    }
    { const std::string m = stream_out_checks("bp_stream_push", due, out_cap, out_pcm); if (!m.empty()) return fail(BP_ERR_ARG, m); }
    if (rows > h->cap)
        return fail(BP_ERR_ARG, "bp_stream_push: " + std::to_string(rows) + " rows (frames + context-1 per active channel) exceed the chunk capacity " +
                                std::to_string(h->cap));
    if ((size_t)n_enh > s->max_enh) return fail(BP_ERR_STATE, "bp_stream_push: internal: more frames than the stream was sized for");
    HIPCHK(hipSetDevice(h->cfg.device));
    float *rows_d = nullptr, *nat_d = nullptr; int *tab_d = nullptr;
    if (n > 0) {
        int r;
        // the noise-aware rows: one per channel, or (dyn) one per sample of the chunk
        const size_t nat_b = !s->nat ? 0 : s->dyn ? (size_t)n * D * 4 : (size_t)nc * D * 4;
        if ((r = window_reserve(h, (size_t)rows * D * 4, 0, nat_b, (size_t)n, &rows_d, nullptr, &nat_d, &tab_d)) != BP_OK) return r;
        if ((r = out_chunk_reserve(h, (int)n)) != BP_OK) return r;
    }
    // ---- the input block: analysis jobs | NAT jobs | synthesis jobs | samples, each 256-byte aligned (the pinned block is reused
    // by every push: the previous one ended in a synchronisation); with it the channels' new state
    s->ana.clear(); s->natj.clear(); s->dnatj.clear(); s->syn.clear();
    Layout ib;
    const size_t o_ana = ib.take((size_t)ana_max * sizeof(AnaJob)), o_nat = ib.take((size_t)active * sizeof(NatJob));
    const size_t o_syn = ib.take((size_t)n_enh * sizeof(SynJob)), o_pcm = ib.size();
    char *pin = s->blk.pin_in.as<char>(), *dev = s->blk.dev.as<char>();
    float *hp = (float *)(pin + o_pcm);
    size_t unit = 0, src = 0;
    int64_t y0 = 0, srow = 0, out_base = 0;
    for (int c = 0; c < nc; ++c) {
        const ChanPlan &p = s->plan[c];
        Chan &ch = s->ch[c];
        const float *in = pcm ? pcm + src : nullptr;
        src += (size_t)n_in[c];
        const int64_t fi0 = p.c0.fi, fi1 = p.c1.fi, fo0 = p.c0.fo, fo1 = p.c1.fo, nf = fi1 - fi0, ne = fo1 - fo0;
        if (nf > 0) {
            // [carry | new] at hop unit `unit`, zeros behind a sentence's end: frame t starts at unit + t - fi0
            ch.carry.fill_segment(hp + unit * hop, (size_t)(nf + 1) * hop, in, (size_t)n_in[c]);
            const int64_t base0 = std::max<int64_t>(0, fo0 - toff), base1 = std::max<int64_t>(0, fo1 - toff), T = fi1;
            const int64_t srows = ne > 0 ? ne + ctx - 1 : 0;
            const int slot0 = (ch.par * nc + c) * R, slot1 = ((ch.par ^ 1) * nc + c) * R;
            for (int64_t t = base0; t < fi1; ++t) {
                AnaJob j; memset(&j, 0, sizeof(j));
                // staged row u of the channel holds frame clamp(fo0 - toff + u, 0, T - 1) (the upper clamp only at the end)
                int64_t lo = t == 0 ? 0 : t - fo0 + toff, hi = (p.ended && t == T - 1) ? srows : t - fo0 + toff + 1;
                lo = std::max<int64_t>(lo, 0); hi = std::min(hi, srows);
                if (lo < hi) { j.stage_lo = (int)(srow + lo); j.stage_hi = (int)(srow + hi); }
                j.state_dst = (!p.ended && t >= base1) ? slot1 + (int)(t - base1) : -1;
                const bool now = t >= fo0 && t < fo1;
                j.g = now ? (int)(p.g0 + t - fo0) : -1; j.y = (int)(y0 + t - fo0); j.ws = (int)(srow + t - fo0); j.chan = c;
                j.y_state = (!p.ended && t >= fo1) ? j.state_dst : -1;
                if (t >= fi0) j.src = (int)(unit + (size_t)(t - fi0));
                else {
                    if (lo >= hi && j.state_dst < 0) continue;      // an old frame nobody needs any more
                    j.src = -1 - (slot0 + (int)(t - base0)); j.has_y = t >= fo0;
                }
                s->ana.push_back(j);
            }
            if (s->dyn) {
                if (ne > 0) {
                    DnatJob j; memset(&j, 0, sizeof(j));
                    j.chan = c; j.t0 = (int)fo0; j.ne = (int)ne; j.y = (int)y0; j.g = (int)p.g0; j.ni = (int)std::min<int64_t>(fi1, 6);
                    j.st = slot1 + (int)(fo1 - base1); j.ended = p.ended;
                    s->dnatj.push_back(j);
                }
            } else if (s->nat) {
                const bool known0 = fi0 >= 6, known1 = p.ended || fi1 >= 6;
                NatJob j; memset(&j, 0, sizeof(j));
                j.chan = c; j.stage = ne > 0;
                if (!known0 && known1) {
                    j.nf = (int)std::min<int64_t>(fi1, 6);
                    if (ne > 0) { j.mode = 0; j.src = (int)(srow + toff); } else { j.mode = 1; j.src = slot1; }
                    s->natj.push_back(j);
                } else if (known0 && ne > 0) { j.mode = 2; s->natj.push_back(j); }
            }
            for (int64_t t = fo0; t < fo1; ++t) {
                SynJob j; memset(&j, 0, sizeof(j));
                j.g = (int)(p.g0 + t - fo0); j.y = (int)(y0 + t - fo0);
                j.prev = t == 0 ? -1 : t == fo0 ? 1 : 0;
                j.half_src = ch.hpar * nc + c;
                j.out_off = (int)(out_base + (t - 1) * hop - p.c0.so);
                j.out_n = t == 0 ? 0 : (int)std::min<int64_t>(hop, p.c1.so - (t - 1) * hop);
                j.half_dst = (!p.ended && t == fo1 - 1) ? (ch.hpar ^ 1) * nc + c : -1;
                s->syn.push_back(j);
            }
            unit += (size_t)(nf + 1);
            y0 += ne; srow += srows; out_base += p.c1.so - p.c0.so;
            ch.par ^= 1;
            if (ne > 0) ch.hpar ^= 1;
        }
        n_out[c] = (int)(p.c1.so - p.c0.so);
        // the carry: the last hop + r1 % hop samples of [carry | new]; a new sentence starts from hop zeros
        if (p.ended) ch.carry.reset(hop);
        else if (n_in[c] > 0 && !ch.carry.keep_last(in, (size_t)n_in[c], (size_t)hop + (size_t)(p.r1 % hop)))
            return fail(BP_ERR_STATE, "bp_stream_push: internal: the carry exceeds its capacity");
    }
    if (s->ana.empty()) return BP_OK;                               // nothing became a frame: no device work
    const size_t in_bytes = o_pcm + unit * hop * 4;
    memcpy(pin + o_ana, s->ana.data(), s->ana.size() * sizeof(AnaJob));
    if (!s->natj.empty()) memcpy(pin + o_nat, s->natj.data(), s->natj.size() * sizeof(NatJob));
    if (!s->dnatj.empty()) memcpy(pin + o_nat, s->dnatj.data(), s->dnatj.size() * sizeof(DnatJob));
    if (!s->syn.empty()) memcpy(pin + o_syn, s->syn.data(), s->syn.size() * sizeof(SynJob));
    char *din = dev + s->o_in;
    HIPCHK(hipMemcpyAsync(din, pin, in_bytes, hipMemcpyHostToDevice, h->stream));
    const float *win = (const float *)(dev + s->o_win);
    const float2 *tw = (const float2 *)(dev + s->o_tw);
    float2 *Y = (float2 *)(dev + s->o_pY);
    {
        StreamAnaArgs a; memset(&a, 0, sizeof(a));
        a.jobs = (const AnaJob *)(din + o_ana); a.pcm = (const float *)(din + o_pcm); a.win = win; a.tw = tw;
        a.mean = (const float *)(dev + s->o_mean); a.inv_std = (const float *)(dev + s->o_istd);
        a.log2M = s->log2M; a.D = D; a.hop = hop;
        a.st_rows = (float *)(dev + s->o_rows); a.st_Y = (float2 *)(dev + s->o_Y);
        a.rows = rows_d; a.Y = Y; a.win_start = tab_d; a.nat_row = (s->nat && n > 0) ? tab_d + 2 * n : nullptr; a.nat_frame = s->dyn;
        // fillers between the channels: window 0, NAT row 0 (the first channel with frames staged at least `context` rows)
        if (n > n_enh) HIPCHK(hipMemsetAsync(tab_d, 0, (size_t)3 * n * sizeof(int), h->stream));
        hipLaunchKernelGGL(bp_stream_analysis, dim3((unsigned)s->ana.size()), dim3(WAVE_THREADS), lds_bytes(hop), h->stream, a);
        HIPCHK(hipGetLastError());
    }
    if (!s->natj.empty()) {
        const int kb = (D + WAVE_THREADS - 1) / WAVE_THREADS;
        hipLaunchKernelGGL(bp_stream_nat, dim3((unsigned)(kb * s->natj.size())), dim3(WAVE_THREADS), 0, h->stream, (const NatJob *)(din + o_nat),
                           (const float *)rows_d, (const float *)(dev + s->o_rows), D, (float *)(dev + s->o_nat), nat_d);
        HIPCHK(hipGetLastError());
    }
    if (!s->dnatj.empty()) {
        StreamDnatArgs a; memset(&a, 0, sizeof(a));
        a.jobs = (const DnatJob *)(din + o_nat); a.Y = Y; a.st_Y = (const float2 *)(dev + s->o_Y);
        a.mean = (const float *)(dev + s->o_mean); a.inv_std = (const float *)(dev + s->o_istd);
        a.lam = (double *)(dev + s->o_lam); a.pb = (double *)(dev + s->o_pb); a.nat = nat_d; a.D = D; a.np = s->nat_np;
        const int kb = (D + DNAT_THREADS - 1) / DNAT_THREADS;
        hipLaunchKernelGGL(bp_stream_dnat, dim3((unsigned)(kb * s->dnatj.size())), dim3(DNAT_THREADS), 0, h->stream, a);
        HIPCHK(hipGetLastError());
    }
    if (n > 0) {
        int r;
        if ((r = window_adopt(h, (int)n, D, ctx, s->nat, false)) != BP_OK) return r;
        if ((r = forward_resident_as(h, (int)n, s->packed ? BP_FORWARD_ROWINV : BP_FORWARD_DEFAULT)) != BP_OK) return r;
        StreamSynArgs a; memset(&a, 0, sizeof(a));
        a.jobs = (const SynJob *)(din + o_syn); a.out = h->out_chunk.as<float>(); a.ldo = h->ld[L - 1]; a.out_col = s->out_col;
        a.Y = Y; a.win = win; a.tw = tw; a.log2M = s->log2M; a.D = D; a.target = s->target;
        a.half = (float *)(dev + s->o_half); a.pcm = (float *)(dev + s->o_out);
        const size_t lds = (syn_frames_at(hop) + (size_t)4 * hop) * sizeof(float);
        if (s->post) hipLaunchKernelGGL(bp_stream_synthesis<PostFn>, dim3((unsigned)n_enh), dim3(WAVE_THREADS), lds, h->stream, a, PostFn{s->pp, s->pp.mask_col - s->out_col});
        else hipLaunchKernelGGL(bp_stream_synthesis<NoPost>, dim3((unsigned)n_enh), dim3(WAVE_THREADS), lds, h->stream, a, NoPost());
        HIPCHK(hipGetLastError());
    }
    HIPCHK(s->blk.copy_back(s->o_out, due, out_pcm, h->stream));
    return BP_OK;
}
