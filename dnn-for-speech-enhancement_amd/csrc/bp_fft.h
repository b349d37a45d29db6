// bp_fft.h -- what the signal-layer translation units share (bp_wave.hip: enhancement and LPS features; bp_mix.hip: training
// mixtures made on the device; bp_eval.hip: objective scores; bp_stream.hip and bp_classic.hip: streams and the log-MMSE baseline):
// on the device the real FFT of one analysis frame in LDS, the synthesis of a frame, the overlap-add and its clipped store; on the
// host the frame plan of a call with its padded layout, the analysis kernel's arguments and the launchers of the bp_wave.hip
// kernels.  Internal: nothing in here is part of the C ABI.
//
// Signal definition: n_fft = 2 (fea_dim - 1) = 2M, hop = M, periodic Hamming window.  A real frame of 2M
// samples is transformed as a complex FFT of M points z[m] = (x[2m], x[2m+1]) followed by the split step.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "bp_handle.h"

namespace {

constexpr int WAVE_THREADS = 256;
constexpr float LN_FLOOR = -23.025850929940457f;   // ln(1e-10)

// LDS index of complex point i: one float2 of padding after every 32, so that the power-of-two strides of the butterfly
// stages (and the bit-reversed scatter) do not pile up on a few banks of ds_read_b64 / ds_write_b64.
__device__ __forceinline__ int lp(int i) { return i + (i >> 5); }
__host__ __device__ inline size_t lds_bytes(int M) { return (size_t)(M + M / 32 + 1) * sizeof(float2); }

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a * conj(b)

// Radix-2 decimation-in-time FFT of M points in LDS (input in bit-reversed order).  tw[j] = exp(-2 pi i j / n_fft), n_fft = 2M;
// inverse: conjugated twiddles, no scaling.
__device__ void fft_lds(float2 *z, int M, const float2 *__restrict__ tw, bool inverse)
{
    for (int h = 1; h < M; h <<= 1) {
        const int tstep = M / h;                                // exp(-2 pi i (j%h) / (2h)) = tw[(j%h) * (2M / (2h))]
        for (int j = threadIdx.x; j < M / 2; j += blockDim.x) {
            const int jh = j & (h - 1), i0 = ((j - jh) << 1) + jh, i1 = i0 + h;
            const float2 w = tw[jh * tstep];
            const float2 a = z[lp(i0)], bb = z[lp(i1)];
            const float2 b = inverse ? cmulc(bb, w) : cmul(bb, w);
            z[lp(i0)] = make_float2(a.x + b.x, a.y + b.y);
            z[lp(i1)] = make_float2(a.x - b.x, a.y - b.y);
        }
        __syncthreads();
    }
}

// Sentence of global frame g: the last s with F[s] <= g (F[n_sent] = all frames).  Uniform per workgroup.
__device__ __forceinline__ int sentence_of(const int *__restrict__ F, int n_sent, int g)
{
    int lo = 0, hi = n_sent - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (F[mid] <= g) lo = mid; else hi = mid - 1; }
    return lo;
}

// Forward real FFT of the 2M samples at x (16-byte aligned) times the window: leaves Z = FFT_M(z) in LDS (natural order, lp
// indexing) for rfft_bin.  Ends with a barrier.
__device__ __forceinline__ void rfft_frame(float2 *z, const float *__restrict__ x, const float *__restrict__ win, const float2 *__restrict__ tw,
                                           int log2M)
{
    const int M = 1 << log2M, N = 2 * M;
    // windowed samples as M complex points z[m] = (x[2m], x[2m+1]), scattered to bit-reversed positions; 16-byte loads
    for (int q = threadIdx.x; q < N / 4; q += blockDim.x) {
        const float4 v = *reinterpret_cast<const float4 *>(x + 4 * q), w = *reinterpret_cast<const float4 *>(win + 4 * q);
        const int m0 = 2 * q, m1 = 2 * q + 1;
        z[lp((int)(__brev((unsigned)m0) >> (32 - log2M)))] = make_float2(v.x * w.x, v.y * w.y);
        z[lp((int)(__brev((unsigned)m1) >> (32 - log2M)))] = make_float2(v.z * w.z, v.w * w.w);
    }
    __syncthreads();
    fft_lds(z, M, tw, false);
}

// split step: X[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[M-k]) / 2, O = (Z[k] - conj Z[M-k]) / 2i, k = 0 .. M
// (the contraction is spelled out, as in overlap4: left to itself the compiler folds the halving of E and one product of W^k O
// into the sums in the analysis kernels, and folds neither where the call sits in other code; every caller must return these bits)
__device__ __forceinline__ float2 rfft_bin(const float2 *z, const float2 *__restrict__ tw, int M, int k)
{
#pragma clang fp contract(off)
    const float2 zk = z[lp(k & (M - 1))], zm = z[lp((M - k) & (M - 1))];
    const float2 o = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
    return k == 0 ? make_float2(zk.x + zk.y, 0.0f) : k == M ? make_float2(zk.x - zk.y, 0.0f)
                                                          : make_float2(fmaf(zk.x + zm.x, 0.5f, fmaf(o.x, tw[k].x, -(o.y * tw[k].y))),
                                                                        fmaf(zk.y - zm.y, 0.5f, fmaf(o.x, tw[k].y, o.y * tw[k].x)));
}

// the LPS of one bin's power, with the 1e-10 floor
__device__ __forceinline__ float lps_of(float p) { return p > 1e-10f ? logf(p) : LN_FLOOR; }

// The power of one noisy bin as bp_wave_analysis forms it (there the compiler multiplies the pair with one packed multiply and adds:
// two squares, each rounded, and their rounded sum; spelled out, uncontracted, for the code that makes the noisy LPS again from the
// stored spectrum, so that it returns those bits wherever it sits)
__device__ __forceinline__ float power_of(float2 X)
{
#pragma clang fp contract(off)
    const float a = X.x * X.x, b = X.y * X.y;
    return a + b;
}

// One post-processed value (bp_set_post; include/bp_c_api.h): x the LPS estimate, m the mask estimate (read
// only with the gate), y the noisy LPS, k the bin.  GV equalisation, then the gate; every step one fp32 operation, rounded once.
__device__ __forceinline__ float post_value(const PostP &p, float x, float m, float y, int k)
{
#pragma clang fp contract(off)
    if (p.gv) {
        const float c = p.c[k], d = x - c, t = p.s[k] * d;
        x = c + t;
    }
    if (p.gate) {
        float u;
        if (p.hi > p.lo) {
            u = (m - p.lo) * p.inv;
            u = u > 0.0f ? (u < 1.0f ? u : 1.0f) : 0.0f;         // (a NaN mask: 0)
        } else
            u = m >= p.hi ? 1.0f : 0.0f;
        const float w = p.weight * u, e = y - x, q = w * e;
        x = x + q;
    }
    return x;
}

// What synth_frame takes for ok = o[k]: the net's column itself, or the post-processed value of it, of the mask column moff columns
// further on and of the noisy LPS made from Y[k]
struct NoPost {
    __device__ __forceinline__ float operator()(float ok, const float *, int, float2) const { return ok; }
};
struct PostFn {
    PostP p; int moff;
    __device__ __forceinline__ float operator()(float ok, const float *__restrict__ o, int k, float2 y) const
    {
        return post_value(p, ok, p.gate ? o[moff + k] : 0.0f, lps_of(power_of(y)), k);
    }
};

// Synthesis of one frame (bp_wave_synthesis, bp_stream_synthesis): S from the net outputs o[0 .. M] and the noisy spectrum
// Y[0 .. M], inverse real FFT, times the window -> fr[0 .. 2M) (16-byte aligned; global or LDS).  z: lds_bytes(M) of FFT space
// followed by M + 1 float2 for S.  Every thread of the workgroup calls it; no barrier behind the stores to fr.  post: what stands
// for o[k] (NoPost: o[k]).
template <class Post = NoPost>
__device__ __forceinline__ void synth_frame(float2 *z, const float *__restrict__ o, const float2 *__restrict__ Y, const float *__restrict__ win,
                                            const float2 *__restrict__ tw, int log2M, int target, float *fr, const Post post = Post())
{
    const int M = 1 << log2M, N = 2 * M, tid = threadIdx.x;
    float2 *S = z + lds_bytes(M) / sizeof(float2);      // S[0 .. M], unpadded (read twice below, written once)
    for (int k = tid; k <= M; k += blockDim.x) {
        const float2 y = Y[k];
        const float ok = post(o[k], o, k, y);
        float2 v;
        if (target == BP_WAVE_MASK) v = make_float2(ok * y.x, ok * y.y);
        else {
            const float r = sqrtf(y.x * y.x + y.y * y.y), m = expf(0.5f * ok);
            v = r > 0.0f ? make_float2(m * (y.x / r), m * (y.y / r)) : make_float2(m, 0.0f);
        }
        if (k == 0 || k == M) v.y = 0.0f;               // (irfft ignores the imaginary part of DC and Nyquist)
        S[k] = v;
    }
    __syncthreads();
    // inverse split step: Z[k] = E[k] + i O[k], E = (S[k] + conj S[M-k]) / 2, O = (S[k] - conj S[M-k]) conj(W^k) / 2
    for (int k = tid; k < M; k += blockDim.x) {
        const float2 sk = S[k], sm = S[M - k];
        const float2 e = make_float2(0.5f * (sk.x + sm.x), 0.5f * (sk.y - sm.y));
        const float2 d = make_float2(0.5f * (sk.x - sm.x), 0.5f * (sk.y + sm.y));
        const float2 od = cmulc(d, tw[k]);
        z[lp((int)(__brev((unsigned)k) >> (32 - log2M)))] = make_float2(e.x - od.y, e.y + od.x);
    }
    __syncthreads();
    fft_lds(z, M, tw, true);
    const float sc = 1.0f / (float)M;
    for (int q = tid; q < N / 4; q += blockDim.x) {
        const float2 z0 = z[lp(2 * q)], z1 = z[lp(2 * q + 1)];
        const float4 w = *reinterpret_cast<const float4 *>(win + 4 * q);
        *reinterpret_cast<float4 *>(fr + 4 * q) = make_float4(z0.x * sc * w.x, z0.y * sc * w.y, z1.x * sc * w.z, z1.y * sc * w.w);
    }
}

// Least-squares overlap-add of four samples: a from the frame that starts at the segment, b from the second half of the frame
// before it, wa / wb the window values at those offsets
__device__ __forceinline__ float4 overlap4(float4 a, float4 b, float4 wa, float4 wb)
{
    // (the fused multiply-add is spelled out: which of the two squares the compiler would fuse depends on the code around the
    // call, and both callers must return the same bits)
    return make_float4((a.x + b.x) / fmaf(wa.x, wa.x, wb.x * wb.x), (a.y + b.y) / fmaf(wa.y, wa.y, wb.y * wb.y),
                       (a.z + b.z) / fmaf(wa.z, wa.z, wb.z * wb.z), (a.w + b.w) / fmaf(wa.w, wa.w, wb.w * wb.w));
}

// The overlap-add of one segment of hop samples into a compact output that is only 4-byte aligned (bp_stream_synthesis,
// bp_lmstream_push): cur the frame that starts at the segment, prev_half the second half of the frame before it; the first n
// samples are stored (n >= hop: all of them; n <= 0: none), one scalar store each.  Every thread of the workgroup calls it;
// threads: their number, spelled as the caller's own loops spell it (blockDim.x or WAVE_THREADS), so that each kernel keeps its code.
__device__ __forceinline__ void overlap_store(const float *cur, const float *prev_half, const float *__restrict__ win, int hop, float *dst, int n,
                                              int threads)
{
    for (int q = threadIdx.x; q < hop / 4; q += threads) {
        const float4 x = *reinterpret_cast<const float4 *>(cur + 4 * q), b = *reinterpret_cast<const float4 *>(prev_half + 4 * q);
        const float4 wa = *reinterpret_cast<const float4 *>(win + 4 * q), wb = *reinterpret_cast<const float4 *>(win + hop + 4 * q);
        const float4 r = overlap4(x, b, wa, wb);
        const int i = 4 * q;
        if (i < n) dst[i] = r.x;
        if (i + 1 < n) dst[i + 1] = r.y;
        if (i + 2 < n) dst[i + 2] = r.z;
        if (i + 3 < n) dst[i + 3] = r.w;
    }
}

// Half a frame (hop samples, 16-byte aligned at both ends) between the LDS frames and a channel's carried half
__device__ __forceinline__ void copy_half(float *dst, const float *src, int hop, int threads)
{
    for (int q = threadIdx.x; q < hop / 4; q += threads)
        *reinterpret_cast<float4 *>(dst + 4 * q) = *reinterpret_cast<const float4 *>(src + 4 * q);
}

}  // namespace

// bp_wave_analysis arguments (bp_wave.hip): frame g of sentence s reads the padded samples [(g + s) hop, (g + s) hop + n_fft).
struct WaveAnaArgs {
    const float *pcm; const float *win; const float2 *tw; const int *F; const float *mean, *inv_std;
    int n_sent, log2M, D, hop, ctx, toff;
    float2 *Y;            // [frames][D] noisy spectrum, or null
    float *lps;           // [frames][D] un-normalised LPS, or null
    float *rows;          // staged normalised rows [frames + n_sent (ctx - 1)][D], or null
    int *win_start, *nat_row;   // [frames] window tables of the chunk (with rows)
    int nat_frame;        // nat_row[g] = the sentence (0: one noise-aware row per sentence) or g itself (1: one per frame, bp_wave_dnat)
};

// Host side of bp_wave.hip, for the other signal-layer units
int wave_log2_fft(int fea_dim);                                   // log2 of M, or -1 outside 1d's range
// Frame plan of a call: T_s = (sent_len[s] - 1) / hop + 2 frames per sentence, F = prefix sums; in the padded layout sentence s
// has T_s + 1 segments of hop samples and its first sample lies at (F[s] + s + 1) hop.  plan_waves checks (fea_dim, the
// pointers, no empty sentence, at most max_frames frames) before any device work, with the caller's name in the messages.
struct WavePlan {
    int M, N, hop, log2M, n_sent;
    std::vector<int> F;                                  // [n_sent + 1]
    size_t frames, padded;                               // frames of the call, padded samples of a PCM buffer
};
int plan_waves(const char *who, int fea_dim, int n_sent, const int *sent_len, const float *pcm, size_t max_frames, WavePlan &p);
void wave_scatter(float *dst, const WavePlan &p, const int *sent_len, const float *pcm);   // the sentences to their padded places (dst: zeros)
void wave_gather(float *out, const WavePlan &p, const int *sent_len, const float *src);    // ... and back, the padding trimmed
// The single host->device block of a call: F | mean | inv_std | window | twiddles | padded PCM, each 256-byte aligned; filled on the
// host (mean null: no norm file; window and twiddles as wave_window_twiddles makes them)
struct WaveIn { size_t F, mean, istd, win, tw, pcm, bytes; };
WaveIn wave_in_layout(const WavePlan &p, int D);
void wave_in_fill(char *hb, const WaveIn &w, const WavePlan &p, int D, const float *mean, const float *inv_std, const int *sent_len,
                  const float *pcm);
void wave_window_twiddles(int log2M, float *win, float2 *tw);     // win[2M], tw[M + 1], computed in double and rounded once
// the grow-only buffers of a signal-layer call, device or pinned host, used by what is queued on h->stream
static inline int wave_grow(bp_handle *h, std::initializer_list<Grow> list) { return grow_all("signal-layer buffers: ", {h->stream}, list); }
hipError_t wave_analysis_launch(const WaveAnaArgs &a, int frames, hipStream_t st);
hipError_t wave_nat_launch(const float *rows, const int *F, int n_sent, int D, int ctx, int toff, float *nat, hipStream_t st);
// the dynamic noise-aware rows: nat [frames][D] from the noisy spectrum Y [frames][D], one row per frame
hipError_t wave_dnat_launch(const NoiseP &np, const float2 *Y, const int *F, int n_sent, int D, const float *mean, const float *inv_std,
                            float *nat, hipStream_t st);
// The noise-aware block of a staging call on h (bp_set_nat): *dyn = one tracked row per frame.  BP_ERR_ARG in the caller's name when
// the handle is in BP_NAT_DYNAMIC and the net has no block (nat == false).
int wave_nat_mode(const char *who, const bp_handle *h, bool nat, bool *dyn);
// synthesis of `frames` frames from the net outputs out[frames][ldo] (columns [out_col, out_col + D)) and Y -> syn[frames][n_fft];
// post: from the post-processed value of those columns (bp_set_post), or null
hipError_t wave_synthesis_launch(const float *out, int ldo, int out_col, const float2 *Y, const float *win, const float2 *tw, int log2M,
                                 int D, int target, float *syn, int frames, hipStream_t st, const PostP *post = nullptr);
// The post-processing of a call that resynthesises with h's net (bp_set_post): BP_OK while it is off; on, BP_ERR_ARG in the caller's
// name when the call's fea_dim is not the one that was set or its target is BP_WAVE_MASK
int wave_post_check(const char *who, const bp_handle *h, int fea_dim, int target);
// the sums of bp_gv_mix (include/bp_c_api.h) over n frames: e from out (post: post-processed with Y's noisy LPS) and r from ref
// [n][D], through h->gv_parts; sums: 4 D doubles on the device (est_sum | est_sq | ref_sum | ref_sq)
hipError_t wave_gv_launch(bp_handle *h, const float *out, int ldo, int out_col, const float2 *Y, const float *ref, int D, int n,
                          const PostP *post, hipStream_t st);
// overlap-add of those frames into the padded layout (segment 0 and segment T of every sentence are not written)
hipError_t wave_overlap_launch(const float *syn, const float *win, const int *F, int n_sent, int hop, float *pcm, int frames, hipStream_t st);
