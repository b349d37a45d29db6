// bp_wave.hip -- C-ABI implementation (include/bp_c_api.h): the signal layer around the network.  Noisy PCM
// in, enhanced PCM out (bp_enhance_waves), and the same analysis alone for feature extraction (bp_wave_lps).  gfx950 only.
//
// One signal definition, derived from fea_dim: n_fft = 2 (fea_dim - 1), a power of two in 64 .. 2048;
// hop = n_fft / 2; periodic Hamming window for analysis and synthesis; a sentence of n samples is padded with n_fft - hop
// zeros in front and zeros behind, and has T = (n - 1) / hop + 2 frames, frame t covering padded samples [t hop, t hop + n_fft).
//
// Device layout of one call (everything in ONE host->device copy, `WaveIn`): sentence s occupies the padded samples
// [(F_s + s) hop, (F_s + s + T_s + 1) hop) of the PCM buffer, F_s = frames of the sentences before it, so frame t of sentence s
// -- global frame g = F_s + t -- starts at sample (g + s) hop: aligned, contiguous, no predicates.  The enhanced samples come
// back in the same padded layout (one device->host copy) and the host trims the padding.  The plan and the layout (plan_waves,
// wave_scatter / wave_gather, wave_in_layout / wave_in_fill) are declared in bp_fft.h: bp_classic.hip and bp_eval.hip use them too.
//
// Kernels (one workgroup of 256 threads = 4 wave64 per frame; the frame's FFT lives in LDS):
//   bp_wave_analysis   window, real FFT of n_fft points as a complex FFT of n_fft/2 points + the split step, then per bin:
//                      the noisy spectrum Y, ln(max(|Y|^2, 1e-10)), the normalised row written where bp_stage_bunch reads it
//                      (the replicated edge rows included), the window chunk's win_start / nat_row entries
//   bp_wave_nat        the noise-aware row of every sentence (mean of its first 6 normalised frames, PfileReader::try_nat_rows order)
//   bp_wave_dnat       BP_NAT_DYNAMIC (bp_set_nat) instead: one noise-aware row per frame, the MMSE-SPP tracker's noise PSD
//   bp_wave_synthesis  per frame: S from the net output and Y, inverse real FFT, times the window -> frames [T][n_fft]
//   bp_wave_overlap    per output sample: the sum over the two covering frames / the sum of squared window values (a gather: no
//                      atomics, the same bits on every run)
//   bp_wave_synthesis<PostFn>  the same from the post-processed value of the net's column (bp_set_post, bp_fft.h: post_value)
//   bp_wave_post_rows  that value over caller rows (bp_post_rows); bp_wave_gv_parts / bp_wave_gv_total: the ordered double sums of bp_gv_mix
//   bp_wave_mel        the MFCC auxiliary target (bp_wave_mfcc, bp_set_mix_aux; bp_mel.h): per frame |S|^2 in LDS, one
//                      lane's serial sum in double per mel filter, one lane's serial sum in double per cepstral coefficient
#include <hip/hip_runtime.h>
#include <string.h>
#include <cmath>
#include <string>
#include <vector>

#include "bp_classic.h"
#include "bp_fft.h"
#include "bp_handle.h"
#include "bp_mel.h"

__global__ __launch_bounds__(WAVE_THREADS) void bp_wave_analysis(const WaveAnaArgs a)
{
    extern __shared__ float2 z[];
    const int g = blockIdx.x, M = 1 << a.log2M, tid = threadIdx.x;
    const int s = sentence_of(a.F, a.n_sent, g), t = g - a.F[s], T = a.F[s + 1] - a.F[s];
    rfft_frame(z, a.pcm + (size_t)(g + s) * a.hop, a.win, a.tw, a.log2M);
    const int base = a.F[s] + s * (a.ctx - 1);          // first staged row of the sentence
    for (int k = tid; k <= M; k += blockDim.x) {
        const float2 X = rfft_bin(z, a.tw, M, k);
        const size_t gi = (size_t)g * a.D + k;
        if (a.Y) a.Y[gi] = X;
        const float p = X.x * X.x + X.y * X.y;
        const float l = lps_of(p);
        if (a.lps) a.lps[gi] = l;
        if (a.rows) {
            const float v = (l - a.mean[k]) * a.inv_std[k];
            // staged row base + u holds frame clamp(u - toff, 0, T-1): frame t at u = t + toff, the first frame also at the
            // toff rows in front of it, the last one also at the ctx-1-toff rows behind it
            a.rows[(size_t)(base + t + a.toff) * a.D + k] = v;
            if (t == 0) for (int u = 0; u < a.toff; ++u) a.rows[(size_t)(base + u) * a.D + k] = v;
            if (t == T - 1) for (int u = T + a.toff; u < T + a.ctx - 1; ++u) a.rows[(size_t)(base + u) * a.D + k] = v;
        }
    }
    if (a.rows && tid == 0) { a.win_start[g] = base + t; if (a.nat_row) a.nat_row[g] = a.nat_frame ? g : s; }
}

namespace {
constexpr int DNAT_THREADS = 64, DNAT_AHEAD = 4;
struct DnatArgs { const float2 *Y; const int *F; const float *mean, *inv_std; float *nat; int D; NoiseP np; };
}  // namespace

// The dynamic noise-aware rows: nat[F_s + t][k] = the normalised LPS of the noise PSD that the MMSE-SPP tracker
// holds at frame t of sentence s.  One thread per (sentence, bin), serial over t: the bins are independent (no sum across them,
// no LDS, no barrier), the frames a dependent chain of one double exp, two divisions and one logf.  64-thread workgroups, so that
// n_sent * ceil(D / 64) of them spread over the CUs; the Y of the next DNAT_AHEAD frames is loaded -- from a clamped row, without
// a predicate -- before the chain of the current ones, which does not depend on it.  The noise start is bp_logmmse_gain's with
// init_frames = 6 (ascending t from 0.0), the step lm_dnat (bp_classic.h).
__global__ __launch_bounds__(DNAT_THREADS) void bp_wave_dnat(const DnatArgs a)
{
#pragma clang fp contract(off)
    const int D = a.D, kb = (D + DNAT_THREADS - 1) / DNAT_THREADS, s = blockIdx.x / kb, k = (blockIdx.x % kb) * DNAT_THREADS + threadIdx.x;
    if (k >= D) return;
    const int f0 = a.F[s], T = a.F[s + 1] - f0, ni = T < 6 ? T : 6;
    const float2 *Y = a.Y + (size_t)f0 * D + k;
    float *nat = a.nat + (size_t)f0 * D + k;
    const float mean = a.mean[k], istd = a.inv_std[k];
    float2 cur[DNAT_AHEAD], nxt[DNAT_AHEAD];
#pragma unroll
    for (int j = 0; j < DNAT_AHEAD; ++j) cur[j] = Y[(size_t)(j < T ? j : T - 1) * D];
    double lam = 0.0, pb = 0.0;
    for (int t = 0; t < ni; ++t) lam += lm_power(Y[(size_t)t * D]);
    lam = lm_noise_start(lam, ni);
    for (int t0 = 0; t0 < T; t0 += DNAT_AHEAD) {
#pragma unroll
        for (int j = 0; j < DNAT_AHEAD; ++j) { const int t = t0 + DNAT_AHEAD + j; nxt[j] = Y[(size_t)(t < T ? t : T - 1) * D]; }
#pragma unroll
        for (int j = 0; j < DNAT_AHEAD; ++j)
            if (t0 + j < T) nat[(size_t)(t0 + j) * D] = lm_dnat(a.np, cur[j], lam, pb, mean, istd);
#pragma unroll
        for (int j = 0; j < DNAT_AHEAD; ++j) cur[j] = nxt[j];
    }
}

// nat[s][k] = ((((v0 + v1) + v2) + v3) + v4 + v5) / 6 over the sentence's first 6 normalised frames, frame f clamped to T-1
__global__ __launch_bounds__(WAVE_THREADS) void bp_wave_nat(const float *__restrict__ rows, const int *__restrict__ F, int D, int ctx,
                                                         int toff, float *__restrict__ nat)
{
    const int kb = (D + WAVE_THREADS - 1) / WAVE_THREADS, s = blockIdx.x / kb, k = (blockIdx.x % kb) * WAVE_THREADS + threadIdx.x;
    if (k >= D) return;
    const int T = F[s + 1] - F[s], nf = T < 6 ? T : 6;
    const float *r = rows + (size_t)(F[s] + s * (ctx - 1) + toff) * D + k;
    float acc = 0.0f;
    for (int f = 0; f < 6; ++f) { const float v = r[(size_t)(f < nf ? f : nf - 1) * D]; acc = f == 0 ? v : acc + v; }
    nat[(size_t)s * D + k] = acc / 6.0f;
}

struct WaveSynArgs {
    const float *out; int ldo, out_col;     // net outputs [frames][ldo], columns [out_col, out_col + D)
    const float2 *Y; const float *win; const float2 *tw;
    int log2M, D, target;
    float *frames;                          // [frames][n_fft]: window * irfft(S)
};

// (Post: NoPost, or PostFn with bp_set_post -- the post-processed value stands for the net's column and is written nowhere)
template <class Post>
__global__ __launch_bounds__(WAVE_THREADS) void bp_wave_synthesis(const WaveSynArgs a, const Post post)
{
    extern __shared__ float2 z[];
    const int g = blockIdx.x;
    synth_frame(z, a.out + (size_t)g * a.ldo + a.out_col, a.Y + (size_t)g * a.D, a.win, a.tw, a.log2M, a.target,
                a.frames + ((size_t)g << (a.log2M + 1)), post);
}

// bp_post_rows: the post-processed value over caller rows, one thread per value
__global__ __launch_bounds__(WAVE_THREADS) void bp_wave_post_rows(const float *__restrict__ est, const float *__restrict__ mask,
                                                               const float *__restrict__ y, const PostP p, int D, size_t total,
                                                               float *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * WAVE_THREADS + threadIdx.x;
    if (i >= total) return;
    out[i] = post_value(p, est[i], p.gate ? mask[i] : 0.0f, y[i], (int)(i % (size_t)D));
}

namespace {
constexpr int GV_THREADS = 64;
struct GvArgs {
    const float *out; int ldo, out_col;     // net outputs [n][ldo], columns [out_col, out_col + D)
    const float2 *Y; const float *ref;      // noisy spectrum and clean LPS, [n][D] each
    int D, n, q, post;                      // q = ceil(n / GV_PARTS) frames per part
    PostFn fn;
    double *parts;                          // [GV_PARTS][4][D], then the totals [4][D]
};
}  // namespace

// The part sums of bp_gv_mix (include/bp_c_api.h): workgroup (x, p) holds 64 bins of part p, one thread per bin, serial over the
// part's frames in ascending order -- four double accumulators from 0.0: e, e^2, r, r^2.  The squares are exact in double, so each
// step is one rounded addition, fused or not.
__global__ __launch_bounds__(GV_THREADS) void bp_wave_gv_parts(const GvArgs a)
{
    const int k = blockIdx.x * GV_THREADS + threadIdx.x, part = blockIdx.y;
    if (k >= a.D) return;
    const int g0 = part * a.q, g1 = g0 + a.q < a.n ? g0 + a.q : a.n;
    double es = 0.0, eq = 0.0, rs = 0.0, rq = 0.0;
    for (int g = g0; g < g1; ++g) {
        const float *o = a.out + (size_t)g * a.ldo + a.out_col;
        const float e = a.post ? a.fn(o[k], o, k, a.Y[(size_t)g * a.D + k]) : o[k], r = a.ref[(size_t)g * a.D + k];
        es += (double)e; eq += (double)e * (double)e;
        rs += (double)r; rq += (double)r * (double)r;
    }
    double *dst = a.parts + (size_t)part * 4 * a.D + k;
    dst[0] = es; dst[a.D] = eq; dst[2 * (size_t)a.D] = rs; dst[3 * (size_t)a.D] = rq;
}

// ... and their totals: part 0 + part 1 + ... in ascending order, one thread per (quantity, bin)
__global__ __launch_bounds__(GV_THREADS) void bp_wave_gv_total(double *parts, int D)
{
    const int i = blockIdx.x * GV_THREADS + threadIdx.x;
    if (i >= 4 * D) return;
    double t = parts[i];
    for (int p = 1; p < GV_PARTS; ++p) t += parts[(size_t)p * 4 * D + i];
    parts[(size_t)GV_PARTS * 4 * D + i] = t;
}

// Segment t >= 1 of a sentence (padded samples [t hop, (t+1) hop)) is covered by frame t (offset k) and frame t-1 (offset
// hop + k); segment 0 is front padding.  One workgroup per global frame, 16-byte accesses.
__global__ __launch_bounds__(WAVE_THREADS) void bp_wave_overlap(const float *__restrict__ frames, const float *__restrict__ win,
                                                             const int *__restrict__ F, int n_sent, int hop, float *__restrict__ pcm)
{
    const int g = blockIdx.x, s = sentence_of(F, n_sent, g);
    if (g == F[s]) return;
    const int N = 2 * hop;
    const float *cur = frames + (size_t)g * N, *prev = frames + (size_t)(g - 1) * N + hop;
    float *dst = pcm + (size_t)(g + s) * hop;
    for (int q = threadIdx.x; q < hop / 4; q += blockDim.x) {
        const float4 a = *reinterpret_cast<const float4 *>(cur + 4 * q), b = *reinterpret_cast<const float4 *>(prev + 4 * q);
        const float4 wa = *reinterpret_cast<const float4 *>(win + 4 * q), wb = *reinterpret_cast<const float4 *>(win + hop + 4 * q);
        *reinterpret_cast<float4 *>(dst + 4 * q) = overlap4(a, b, wa, wb);
    }
}

// One frame's power spectrum, log mel energies and cepstral coefficients.  The order of every sum is the
// definition, so no sum is spread over lanes: thread j < n_mel adds the bins of filter j in ascending order to one double, thread
// r < n_ceps the filters in ascending order to another.  A product of two fp32 values is exact in double, so each step is one
// rounded addition, fused or not.  LDS: the FFT, then P[M + 1] and the n_mel log energies.
__global__ __launch_bounds__(WAVE_THREADS) void bp_wave_mel(const MelArgs a)
{
    extern __shared__ float2 z[];
    const int g = blockIdx.x, M = 1 << a.log2M, tid = threadIdx.x;
    float *P = reinterpret_cast<float *>(z + lds_bytes(M) / sizeof(float2)), *lm = P + (M + 1);
    const int s = sentence_of(a.F, a.n_sent, g);
    rfft_frame(z, a.pcm + (size_t)(g + s) * a.hop, a.win, a.tw, a.log2M);
    for (int k = tid; k <= M; k += blockDim.x) {
        const float2 X = rfft_bin(z, a.tw, M, k);
        const float p = X.x * X.x + X.y * X.y;
        P[k] = p;
        if (a.power) a.power[(size_t)g * a.D + k] = p;
    }
    __syncthreads();
    if (tid < a.m.n_mel) {
        const float *w = a.m.wp + a.m.off[tid], *pk = P + a.m.first[tid];
        const int nb = a.m.nb[tid];
        double E = 0.0;
        for (int i = 0; i < nb; ++i) E = fma((double)w[i], (double)pk[i], E);
        const float l = lps_of((float)E);
        lm[tid] = l;
        if (a.logmel) a.logmel[(size_t)g * a.m.n_mel + tid] = l;
    }
    __syncthreads();
    if (a.mfcc && tid < a.m.n_ceps) {
        const float *t = a.m.tT + tid;
        double c = 0.0;
        for (int j = 0; j < a.m.n_mel; ++j) c = fma((double)t[(size_t)j * a.m.n_ceps], (double)lm[j], c);
        a.mfcc[(size_t)g * a.ldm + a.col + tid] = ((float)c - a.m.mean[tid]) * a.m.scale[tid];
    }
}

// ------------------------------------------------------------------ host side
int wave_log2_fft(int fea_dim)
{
    if (fea_dim < 33 || fea_dim > 1025) return -1;
    const int n = 2 * (fea_dim - 1);
    if (n & (n - 1)) return -1;
    int l = 0;
    while ((1 << l) < n) ++l;
    return l - 1;                                        // log2 of M = n_fft / 2
}

void wave_window_twiddles(int log2M, float *win, float2 *tw)
{
    const int M = 1 << log2M, N = 2 * M;
    const double pi2 = 6.283185307179586476925286766559;
    for (int k = 0; k < N; ++k) win[k] = (float)(0.54 - 0.46 * cos(pi2 * k / N));
    for (int k = 0; k <= M; ++k) tw[k] = make_float2((float)cos(pi2 * k / N), (float)-sin(pi2 * k / N));
}

hipError_t wave_analysis_launch(const WaveAnaArgs &a, int frames, hipStream_t st)
{
    hipLaunchKernelGGL(bp_wave_analysis, dim3((unsigned)frames), dim3(WAVE_THREADS), lds_bytes(1 << a.log2M), st, a);
    return hipGetLastError();
}

hipError_t wave_nat_launch(const float *rows, const int *F, int n_sent, int D, int ctx, int toff, float *nat, hipStream_t st)
{
    hipLaunchKernelGGL(bp_wave_nat, dim3((unsigned)(((D + WAVE_THREADS - 1) / WAVE_THREADS) * n_sent)), dim3(WAVE_THREADS), 0, st,
                       rows, F, D, ctx, toff, nat);
    return hipGetLastError();
}

hipError_t wave_dnat_launch(const NoiseP &np, const float2 *Y, const int *F, int n_sent, int D, const float *mean, const float *inv_std,
                            float *nat, hipStream_t st)
{
    DnatArgs a; memset(&a, 0, sizeof(a));
    a.Y = Y; a.F = F; a.mean = mean; a.inv_std = inv_std; a.nat = nat; a.D = D; a.np = np;
    hipLaunchKernelGGL(bp_wave_dnat, dim3((unsigned)(((D + DNAT_THREADS - 1) / DNAT_THREADS) * n_sent)), dim3(DNAT_THREADS), 0, st, a);
    return hipGetLastError();
}

int wave_nat_mode(const char *who, const bp_handle *h, bool nat, bool *dyn)
{
    *dyn = h->nat_mode == BP_NAT_DYNAMIC;
    if (*dyn && !nat)
        return fail(BP_ERR_ARG, std::string(who) + ": the handle is in BP_NAT_DYNAMIC (bp_set_nat) and this net has no noise-aware block: "
                                                   "layersizes[0] is context*fea_dim, not (context+1)*fea_dim");
    return BP_OK;
}

// The noise-aware block of the calls that stage it (include/bp_c_api.h).  Every check before anything is touched.
extern "C" int bp_set_nat(bp_handle *h, int mode, const bp_noise_params *np)
{
    if (!h) return fail(BP_ERR_ARG, "bp_set_nat: null handle");
    if (mode != BP_NAT_STATIC && mode != BP_NAT_DYNAMIC) return fail(BP_ERR_ARG, "bp_set_nat: mode must be BP_NAT_STATIC or BP_NAT_DYNAMIC");
    NoiseP n;
    { const int r = noise_check("bp_set_nat", np, n); if (r != BP_OK) return r; }
    if (mode == BP_NAT_DYNAMIC && !n.spp)
        return fail(BP_ERR_ARG, "bp_set_nat: np->mode must be BP_NOISE_SPP with BP_NAT_DYNAMIC (the VAD-gated update needs the gains of the log-MMSE recursion)");
    h->nat_mode = mode; h->nat_np = n;
    return BP_OK;
}

// ------------------------------------------------------------------ post-processing of the LPS estimate (include/bp_c_api.h)
// The range rules of bp_post_params in the caller's name; sL: the net's output width, or -1 without a net (bp_post_rows: mask_col
// only switches the gate on).  out: everything but the device pointers.
static int post_check(const char *who, int fea_dim, const bp_post_params *p, int sL, PostP &out)
{
    const std::string w(who);
    if (wave_log2_fft(fea_dim) < 0) return fail(BP_ERR_ARG, w + ": 2*(fea_dim-1) must be a power of two from 64 to 2048");
    if (p->gv != 0 && p->gv != 1) return fail(BP_ERR_ARG, w + ": gv must be 0 or 1");
    if (p->gv) {
        if (!p->gv_center || !p->gv_scale) return fail(BP_ERR_ARG, w + ": gv = 1 needs gv_center and gv_scale");
        for (int k = 0; k < fea_dim; ++k) {
            if (!std::isfinite(p->gv_center[k])) return fail(BP_ERR_ARG, w + ": gv_center[" + std::to_string(k) + "] is not finite");
            if (!std::isfinite(p->gv_scale[k]) || !(p->gv_scale[k] > 0.0f))
                return fail(BP_ERR_ARG, w + ": gv_scale[" + std::to_string(k) + "] must be finite and > 0");
        }
    }
    if (p->mask_col < -1) return fail(BP_ERR_ARG, w + ": mask_col must be -1 (no gating) or a column");
    if (sL >= 0 && p->mask_col >= 0 && (long)p->mask_col + fea_dim > sL) return fail(BP_ERR_ARG, w + ": mask_col + fea_dim exceeds layersizes[last]");
    if (!std::isfinite(p->mask_lo) || !std::isfinite(p->mask_hi) || !std::isfinite(p->mask_weight))
        return fail(BP_ERR_ARG, w + ": mask_lo, mask_hi and mask_weight must be finite");
    if (p->mask_lo > p->mask_hi) return fail(BP_ERR_ARG, w + ": mask_lo must not exceed mask_hi");
    if (p->mask_weight < 0.0f || p->mask_weight > 1.0f) return fail(BP_ERR_ARG, w + ": mask_weight outside [0, 1]");
    memset(&out, 0, sizeof(out));
    out.gv = p->gv; out.gate = p->mask_col >= 0; out.mask_col = p->mask_col;
    out.lo = p->mask_lo; out.hi = p->mask_hi; out.weight = p->mask_weight;
    out.inv = p->mask_hi > p->mask_lo ? (float)(1.0 / ((double)p->mask_hi - (double)p->mask_lo)) : 0.0f;
    return BP_OK;
}

extern "C" int bp_post_defaults(bp_post_params *p)
{
    if (!p) return fail(BP_ERR_ARG, "bp_post_defaults: null pointer");
    p->gv = 0; p->gv_center = p->gv_scale = nullptr;
    p->mask_col = -1; p->mask_lo = p->mask_hi = 0.5f; p->mask_weight = 1.0f;
    return BP_OK;
}

// Every check before anything is touched; the device block is allocated by the first call that turns post-processing on, at the
// parameter limit of fea_dim, and never again.
extern "C" int bp_set_post(bp_handle *h, int fea_dim, const bp_post_params *p)
{
    if (!h) return fail(BP_ERR_ARG, "bp_set_post: null handle");
    if (h->dp) return fail(BP_ERR_STATE, "bp_set_post: not on an attached data-parallel handle");
    if (!p) { h->post_on = false; return BP_OK; }
    PostP q;
    { const int r = post_check("bp_set_post", fea_dim, p, h->s[h->L - 1], q); if (r != BP_OK) return r; }
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->post_tab) {
        const int r = dev_alloc(h, &h->post_tab, 2 * (size_t)POST_MAX_D);
        if (r != BP_OK) return r;
    }
    HIPCHK(hipStreamSynchronize(h->stream));                     // (an earlier call's synthesis may still read the block)
    if (q.gv) {
        HIPCHK(hipMemcpy(h->post_tab, p->gv_center, (size_t)fea_dim * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->post_tab + POST_MAX_D, p->gv_scale, (size_t)fea_dim * 4, hipMemcpyHostToDevice));
    }
    q.c = h->post_tab; q.s = h->post_tab + POST_MAX_D;
    h->post = q; h->post_D = fea_dim; h->post_on = true;
    return BP_OK;
}

int wave_post_check(const char *who, const bp_handle *h, int fea_dim, int target)
{
    if (!h->post_on) return BP_OK;
    if (fea_dim != h->post_D)
        return fail(BP_ERR_ARG, std::string(who) + ": post-processing is set for fea_dim " + std::to_string(h->post_D) + " (bp_set_post), not " +
                                    std::to_string(fea_dim));
    if (target == BP_WAVE_MASK) return fail(BP_ERR_ARG, std::string(who) + ": post-processing (bp_set_post) applies to BP_WAVE_LPS, not to BP_WAVE_MASK");
    return BP_OK;
}

extern "C" int bp_post_rows(int device, int fea_dim, int n_frames, const float *est, const float *mask, const float *noisy_lps,
                            const bp_post_params *p, float *out)
{
    if (!p) return fail(BP_ERR_ARG, "bp_post_rows: null parameters");
    PostP q;
    { const int r = post_check("bp_post_rows", fea_dim, p, -1, q); if (r != BP_OK) return r; }
    if (n_frames < 1) return fail(BP_ERR_ARG, "bp_post_rows: n_frames must be >= 1");
    if (!est || !noisy_lps || !out || (q.gate && !mask)) return fail(BP_ERR_ARG, "bp_post_rows: null pointer");
    const size_t total = (size_t)n_frames * fea_dim, row_b = total * 4;
    Layout lay;                                                  // centre | scale | est | mask | noisy LPS, then the output
    const size_t o_c = lay.take((size_t)fea_dim * 4), o_s = lay.take((size_t)fea_dim * 4), o_e = lay.take(row_b);
    const size_t o_m = lay.take(q.gate ? row_b : 0), o_y = lay.take(row_b), o_out = lay.take(row_b);
    OneShot os;
    { const int r = os.open("bp_post_rows", device, lay.size()); if (r != BP_OK) return r; }
    hipError_t &e = os.e;
    char *d = os.d.as<char>();
    if (e == hipSuccess && q.gv) e = hipMemcpyAsync(d + o_c, p->gv_center, (size_t)fea_dim * 4, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess && q.gv) e = hipMemcpyAsync(d + o_s, p->gv_scale, (size_t)fea_dim * 4, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_e, est, row_b, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess && q.gate) e = hipMemcpyAsync(d + o_m, mask, row_b, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_y, noisy_lps, row_b, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess) {
        q.c = (const float *)(d + o_c); q.s = (const float *)(d + o_s);
        hipLaunchKernelGGL(bp_wave_post_rows, dim3((unsigned)((total + WAVE_THREADS - 1) / WAVE_THREADS)), dim3(WAVE_THREADS), 0, os.st,
                           (const float *)(d + o_e), (const float *)(d + o_m), (const float *)(d + o_y), q, fea_dim, total, (float *)(d + o_out));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + o_out, row_b, hipMemcpyDeviceToHost, os.st);
    return os.finish("bp_post_rows");
}

extern "C" int bp_gv_factors(int fea_dim, int64_t frames, const double *est_sum, const double *est_sq, const double *ref_sum, const double *ref_sq,
                             int mode, float *center, float *scale)
{
#pragma clang fp contract(off)                                   // (S2 / n - m * m: two roundings, as the definition has them)
    if (wave_log2_fft(fea_dim) < 0) return fail(BP_ERR_ARG, "bp_gv_factors: 2*(fea_dim-1) must be a power of two from 64 to 2048");
    if (!est_sum || !est_sq || !ref_sum || !ref_sq || !center || !scale) return fail(BP_ERR_ARG, "bp_gv_factors: null pointer");
    if (mode != BP_GV_INDEP && mode != BP_GV_DEP) return fail(BP_ERR_ARG, "bp_gv_factors: mode must be BP_GV_INDEP or BP_GV_DEP");
    if (frames < 2) return fail(BP_ERR_ARG, "bp_gv_factors: need at least 2 frames");
    const double n = (double)frames;
    std::vector<double> ve((size_t)fea_dim), vr((size_t)fea_dim), mr((size_t)fea_dim);
    for (int k = 0; k < fea_dim; ++k) {
        const double me = est_sum[k] / n;
        mr[k] = ref_sum[k] / n;
        ve[k] = est_sq[k] / n - me * me; vr[k] = ref_sq[k] / n - mr[k] * mr[k];
        if (!(ve[k] > 0.0) || !std::isfinite(ve[k])) return fail(BP_ERR_ARG, "bp_gv_factors: the estimate's variance of bin " + std::to_string(k) + " is not > 0");
        if (!(vr[k] > 0.0) || !std::isfinite(vr[k])) return fail(BP_ERR_ARG, "bp_gv_factors: the reference's variance of bin " + std::to_string(k) + " is not > 0");
    }
    double pooled = 0.0;
    for (int k = 0; k < fea_dim; ++k) pooled += ve[k] / vr[k];
    const float beta = (float)sqrt((double)fea_dim / pooled);
    for (int k = 0; k < fea_dim; ++k) {
        center[k] = (float)mr[k];
        scale[k] = mode == BP_GV_DEP ? (float)sqrt(vr[k] / ve[k]) : beta;
    }
    return BP_OK;
}

hipError_t wave_synthesis_launch(const float *out, int ldo, int out_col, const float2 *Y, const float *win, const float2 *tw, int log2M,
                                 int D, int target, float *syn, int frames, hipStream_t st, const PostP *post)
{
    WaveSynArgs a; memset(&a, 0, sizeof(a));
    a.out = out; a.ldo = ldo; a.out_col = out_col;
    a.Y = Y; a.win = win; a.tw = tw; a.log2M = log2M; a.D = D; a.target = target; a.frames = syn;
    const int M = 1 << log2M;
    const size_t lds = lds_bytes(M) + (size_t)(M + 1) * sizeof(float2);
    if (post) hipLaunchKernelGGL(bp_wave_synthesis<PostFn>, dim3((unsigned)frames), dim3(WAVE_THREADS), lds, st, a, PostFn{*post, post->mask_col - out_col});
    else hipLaunchKernelGGL(bp_wave_synthesis<NoPost>, dim3((unsigned)frames), dim3(WAVE_THREADS), lds, st, a, NoPost());
    return hipGetLastError();
}

hipError_t wave_gv_launch(bp_handle *h, const float *out, int ldo, int out_col, const float2 *Y, const float *ref, int D, int n,
                          const PostP *post, hipStream_t st)
{
    GvArgs a; memset(&a, 0, sizeof(a));
    a.out = out; a.ldo = ldo; a.out_col = out_col; a.Y = Y; a.ref = ref; a.D = D; a.n = n; a.q = (n + GV_PARTS - 1) / GV_PARTS;
    if (post) { a.post = 1; a.fn = PostFn{*post, post->mask_col - out_col}; }
    a.parts = reinterpret_cast<double *>(h->gv_parts);
    hipLaunchKernelGGL(bp_wave_gv_parts, dim3((unsigned)((D + GV_THREADS - 1) / GV_THREADS), GV_PARTS), dim3(GV_THREADS), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bp_wave_gv_total, dim3((unsigned)((4 * D + GV_THREADS - 1) / GV_THREADS)), dim3(GV_THREADS), 0, st, a.parts, D);
    return hipGetLastError();
}

hipError_t wave_overlap_launch(const float *syn, const float *win, const int *F, int n_sent, int hop, float *pcm, int frames, hipStream_t st)
{
    hipLaunchKernelGGL(bp_wave_overlap, dim3((unsigned)frames), dim3(WAVE_THREADS), 0, st, syn, win, F, n_sent, hop, pcm);
    return hipGetLastError();
}

hipError_t wave_mel_launch(const MelArgs &a, int frames, hipStream_t st)
{
    const int M = 1 << a.log2M;
    hipLaunchKernelGGL(bp_wave_mel, dim3((unsigned)frames), dim3(WAVE_THREADS), lds_bytes(M) + (size_t)(M + 1 + MEL_MAX) * 4, st, a);
    return hipGetLastError();
}

// Frame plan of a call (bp_fft.h).  Checked before any device work.
int plan_waves(const char *who, int fea_dim, int n_sent, const int *sent_len, const float *pcm, size_t max_frames, WavePlan &p)
{
    p.log2M = wave_log2_fft(fea_dim);
    if (p.log2M < 0) return fail(BP_ERR_ARG, std::string(who) + ": 2*(fea_dim-1) must be a power of two from 64 to 2048");
    if (n_sent < 1 || !sent_len || !pcm) return fail(BP_ERR_ARG, std::string(who) + ": no sentences or null pointer");
    p.M = 1 << p.log2M; p.N = 2 * p.M; p.hop = p.M; p.n_sent = n_sent;
    p.F.assign((size_t)n_sent + 1, 0);
    size_t f = 0;
    for (int s = 0; s < n_sent; ++s) {
        if (sent_len[s] < 1) return fail(BP_ERR_ARG, std::string(who) + ": empty sentence " + std::to_string(s));
        f += (size_t)((sent_len[s] - 1) / p.hop + 2);
        if (f > max_frames) return fail(BP_ERR_ARG, std::string(who) + ": too many frames in one call");
        p.F[s + 1] = (int)f;
    }
    p.frames = f;
    p.padded = (f + (size_t)n_sent) * p.hop;             // sentence s: T_s + 1 segments of hop samples
    return BP_OK;
}

void wave_scatter(float *dst, const WavePlan &p, const int *sent_len, const float *pcm)
{
    for (int s = 0; s < p.n_sent; pcm += sent_len[s++]) memcpy(dst + (size_t)(p.F[s] + s + 1) * p.hop, pcm, (size_t)sent_len[s] * 4);
}

void wave_gather(float *out, const WavePlan &p, const int *sent_len, const float *src)
{
    for (int s = 0; s < p.n_sent; out += sent_len[s++]) memcpy(out, src + (size_t)(p.F[s] + s + 1) * p.hop, (size_t)sent_len[s] * 4);
}

WaveIn wave_in_layout(const WavePlan &p, int D)
{
    WaveIn w;
    Layout lay;
    w.F = lay.take(((size_t)p.n_sent + 1) * 4); w.mean = lay.take((size_t)D * 4); w.istd = lay.take((size_t)D * 4);
    w.win = lay.take((size_t)p.N * 4); w.tw = lay.take((size_t)(p.M + 1) * 8); w.pcm = lay.take(p.padded * 4);
    w.bytes = lay.size();
    return w;
}

void wave_in_fill(char *hb, const WaveIn &w, const WavePlan &p, int D, const float *mean, const float *inv_std, const int *sent_len,
                  const float *pcm)
{
    memcpy(hb + w.F, p.F.data(), p.F.size() * 4);
    if (mean) { memcpy(hb + w.mean, mean, (size_t)D * 4); memcpy(hb + w.istd, inv_std, (size_t)D * 4); }
    wave_window_twiddles(p.log2M, (float *)(hb + w.win), (float2 *)(hb + w.tw));
    float *x = (float *)(hb + w.pcm);
    memset(x, 0, p.padded * 4);
    wave_scatter(x, p, sent_len, pcm);
}

// the most frames of a call that goes through a window chunk or returns LPS rows
static const size_t WAVE_MAX_FRAMES = (size_t)INT32_MAX / 2;

extern "C" int bp_wave_lps(int device, int fea_dim, int n_sent, const int *sent_len, const float *pcm, float *lps)
{
    WavePlan p;
    { const int r = plan_waves("bp_wave_lps", fea_dim, n_sent, sent_len, pcm, WAVE_MAX_FRAMES, p); if (r != BP_OK) return r; }
    if (!lps) return fail(BP_ERR_ARG, "bp_wave_lps: null output");
    const WaveIn w = wave_in_layout(p, fea_dim);
    const size_t out_b = p.frames * fea_dim * 4;
    OneShot os;
    { const int r = os.open("bp_wave_lps", device, w.bytes + out_b); if (r != BP_OK) return r; }
    std::vector<char> hb(w.bytes);
    wave_in_fill(hb.data(), w, p, fea_dim, nullptr, nullptr, sent_len, pcm);
    hipError_t &e = os.e;
    char *d = os.d.as<char>();
    if (e == hipSuccess) e = hipMemcpyAsync(d, hb.data(), w.bytes, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess) {
        WaveAnaArgs a; memset(&a, 0, sizeof(a));
        a.pcm = (const float *)(d + w.pcm); a.win = (const float *)(d + w.win); a.tw = (const float2 *)(d + w.tw); a.F = (const int *)(d + w.F);
        a.n_sent = n_sent; a.log2M = p.log2M; a.D = fea_dim; a.hop = p.hop; a.ctx = 1;
        a.lps = (float *)(d + w.bytes);
        e = wave_analysis_launch(a, (int)p.frames, os.st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(lps, d + w.bytes, out_b, hipMemcpyDeviceToHost, os.st);
    return os.finish("bp_wave_lps");
}

// ------------------------------------------------------------------ the MFCC auxiliary target (include/bp_c_api.h)
extern "C" int bp_mel_defaults(int sample_rate, bp_mel_params *p)
{
    if (!p) return fail(BP_ERR_ARG, "bp_mel_defaults: null pointer");
    if (sample_rate < 1) return fail(BP_ERR_ARG, "bp_mel_defaults: sample_rate must be > 0");
    p->sample_rate = sample_rate; p->n_mel = 26; p->n_ceps = 13; p->first_coef = 0;
    p->f_lo = 0.0f; p->f_hi = 0.5f * (float)sample_rate; p->lifter = 22.0f;
    p->mean = p->scale = nullptr;
    return BP_OK;
}

extern "C" int bp_mel_filters(int fea_dim, const bp_mel_params *p, float *w, int *first_bin, int *n_bins)
{
    MelP m; MelTab tab;
    { const int r = mel_check("bp_mel_filters", p, m); if (r != BP_OK) return r; }
    if (wave_log2_fft(fea_dim) < 0) return fail(BP_ERR_ARG, "bp_mel_filters: 2*(fea_dim-1) must be a power of two from 64 to 2048");
    { const int r = mel_tables("bp_mel_filters", fea_dim, m, tab); if (r != BP_OK) return r; }
    if (w) memcpy(w, tab.w.data(), tab.w.size() * 4);
    if (first_bin) memcpy(first_bin, tab.first.data(), tab.first.size() * 4);
    if (n_bins) memcpy(n_bins, tab.nb.data(), tab.nb.size() * 4);
    return BP_OK;
}

extern "C" int bp_mel_dct(const bp_mel_params *p, float *t)
{
    MelP m;
    { const int r = mel_check("bp_mel_dct", p, m); if (r != BP_OK) return r; }
    if (!t) return fail(BP_ERR_ARG, "bp_mel_dct: null output");
    mel_dct(m, t);
    return BP_OK;
}

extern "C" int bp_wave_mfcc(int device, int fea_dim, const bp_mel_params *mp, int n_sent, const int *sent_len, const float *pcm, float *power,
                            float *logmel, float *mfcc)
{
    MelP m; MelTab tab; WavePlan p;
    { const int r = mel_check("bp_wave_mfcc", mp, m); if (r != BP_OK) return r; }
    { const int r = plan_waves("bp_wave_mfcc", fea_dim, n_sent, sent_len, pcm, WAVE_MAX_FRAMES, p); if (r != BP_OK) return r; }
    { const int r = mel_tables("bp_wave_mfcc", fea_dim, m, tab); if (r != BP_OK) return r; }
    if (!power && !logmel && !mfcc) return fail(BP_ERR_ARG, "bp_wave_mfcc: no output");
    const WaveIn w = wave_in_layout(p, fea_dim);
    const MelBlock mb = mel_block(m.n_mel, m.n_ceps, mel_packed_weights(tab));
    Layout lay(w.bytes);                                         // the input block | the tables | power | logmel | mfcc
    const size_t o_mb = lay.take(mb.bytes), in_b = lay.size();
    const size_t pw_b = power ? p.frames * fea_dim * 4 : 0, lm_b = logmel ? p.frames * m.n_mel * 4 : 0, cc_b = mfcc ? p.frames * m.n_ceps * 4 : 0;
    const size_t o_pw = lay.take(pw_b), o_lm = lay.take(lm_b), o_cc = lay.take(cc_b);
    OneShot os;
    { const int r = os.open("bp_wave_mfcc", device, lay.size()); if (r != BP_OK) return r; }
    std::vector<char> hb(in_b, 0);
    wave_in_fill(hb.data(), w, p, fea_dim, nullptr, nullptr, sent_len, pcm);
    mel_block_fill(hb.data() + o_mb, mb, m, tab);
    hipError_t &e = os.e;
    char *d = os.d.as<char>();
    if (e == hipSuccess) e = hipMemcpyAsync(d, hb.data(), in_b, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess) {
        MelArgs a; memset(&a, 0, sizeof(a));
        a.pcm = (const float *)(d + w.pcm); a.win = (const float *)(d + w.win); a.tw = (const float2 *)(d + w.tw); a.F = (const int *)(d + w.F);
        a.n_sent = n_sent; a.log2M = p.log2M; a.D = fea_dim; a.hop = p.hop;
        a.m = mel_dev(d + o_mb, mb, tab);
        a.power = power ? (float *)(d + o_pw) : nullptr; a.logmel = logmel ? (float *)(d + o_lm) : nullptr;
        a.mfcc = mfcc ? (float *)(d + o_cc) : nullptr; a.ldm = m.n_ceps; a.col = 0;
        e = wave_mel_launch(a, (int)p.frames, os.st);
    }
    if (e == hipSuccess && power) e = hipMemcpyAsync(power, d + o_pw, pw_b, hipMemcpyDeviceToHost, os.st);
    if (e == hipSuccess && logmel) e = hipMemcpyAsync(logmel, d + o_lm, lm_b, hipMemcpyDeviceToHost, os.st);
    if (e == hipSuccess && mfcc) e = hipMemcpyAsync(mfcc, d + o_cc, cc_b, hipMemcpyDeviceToHost, os.st);
    return os.finish("bp_wave_mfcc");
}

extern "C" int bp_enhance_waves(bp_handle *h, int fea_dim, const bp_wave_chunk *c, float *out_pcm, float *out_net)
{
    if (!h || !c) return fail(BP_ERR_ARG, "bp_enhance_waves: null handle or chunk");
    WavePlan p;
    { const int r = plan_waves("bp_enhance_waves", fea_dim, c->n_sent, c->sent_len, c->pcm, WAVE_MAX_FRAMES, p); if (r != BP_OK) return r; }
    if (!out_pcm || !c->mean || !c->inv_std) return fail(BP_ERR_ARG, "bp_enhance_waves: null pointer");
    if (h->dp) return fail(BP_ERR_STATE, "bp_enhance_waves: not on an attached data-parallel handle");
    const int D = fea_dim, ctx = c->context, toff = c->targ_offset, L = h->L, sL = h->s[L - 1];
    if (ctx < 1 || toff < 0 || toff >= ctx) return fail(BP_ERR_ARG, "bp_enhance_waves: need context >= 1 and 0 <= targ_offset < context");
    const bool nat = (long)h->s[0] == (long)(ctx + 1) * D;
    if (!nat && (long)h->s[0] != (long)ctx * D)
        return fail(BP_ERR_ARG, "bp_enhance_waves: layersizes[0] must be context*fea_dim or (context+1)*fea_dim");
    bool dyn;
    { const int r = wave_nat_mode("bp_enhance_waves", h, nat, &dyn); if (r != BP_OK) return r; }
    if (c->target != BP_WAVE_LPS && c->target != BP_WAVE_MASK) return fail(BP_ERR_ARG, "bp_enhance_waves: target must be BP_WAVE_LPS or BP_WAVE_MASK");
    if (c->out_col < 0 || (long)c->out_col + D > sL) return fail(BP_ERR_ARG, "bp_enhance_waves: out_col + fea_dim exceeds layersizes[last]");
    { const int r = wave_post_check("bp_enhance_waves", h, D, c->target); if (r != BP_OK) return r; }
    const size_t rows = p.frames + (size_t)c->n_sent * (ctx - 1);
    if (rows > (size_t)h->cap)
        return fail(BP_ERR_ARG, "bp_enhance_waves: " + std::to_string(rows) + " rows (frames + replicated edge rows) exceed the chunk capacity " +
                                std::to_string(h->cap));
    HIPCHK(hipSetDevice(h->cfg.device));
    const int n = (int)p.frames, N = p.N;
    const WaveIn w = wave_in_layout(p, D);
    const size_t y_b = p.frames * D * sizeof(float2), fr_b = p.frames * N * 4, pcm_b = p.padded * 4;
    int r = wave_grow(h, {{h->wave[0], w.bytes, false}, {h->wave[1], y_b, false}, {h->wave[2], fr_b, false}, {h->wave[3], pcm_b, false},
                          {h->wave_pin[0], w.bytes, true}, {h->wave_pin[1], pcm_b, true}});
    if (r != BP_OK) return r;
    float *rows_d, *nat_d; int *tab_d;
    const size_t nat_b = !nat ? 0 : dyn ? p.frames * D * 4 : (size_t)c->n_sent * D * 4;     // one row per frame | per sentence
    if ((r = window_reserve(h, rows * D * 4, 0, nat_b, p.frames, &rows_d, nullptr, &nat_d, &tab_d)) != BP_OK) return r;
    int *ws_d = tab_d, *nr_d = tab_d + 2 * p.frames;
    if ((r = out_chunk_reserve(h, n)) != BP_OK) return r;      // (forward_resident would; growing it here keeps its sync out of the sequence)
    // The pinned blocks are reused by the next call: the previous call ended in a synchronisation, so nothing still reads them.
    char *hin = (char *)h->wave_pin[0].p, *din = (char *)h->wave[0].p;
    wave_in_fill(hin, w, p, D, c->mean, c->inv_std, c->sent_len, c->pcm);
    HIPCHK(hipMemcpyAsync(din, hin, w.bytes, hipMemcpyHostToDevice, h->stream));
    const float *win = (const float *)(din + w.win);
    const float2 *tw = (const float2 *)(din + w.tw);
    const int *F = (const int *)(din + w.F);
    float2 *Y = (float2 *)h->wave[1].p;
    {
        WaveAnaArgs a; memset(&a, 0, sizeof(a));
        a.pcm = (const float *)(din + w.pcm); a.win = win; a.tw = tw; a.F = F;
        a.mean = (const float *)(din + w.mean); a.inv_std = (const float *)(din + w.istd);
        a.n_sent = c->n_sent; a.log2M = p.log2M; a.D = D; a.hop = p.hop; a.ctx = ctx; a.toff = toff;
        a.Y = Y; a.rows = rows_d; a.win_start = ws_d; a.nat_row = nat ? nr_d : nullptr; a.nat_frame = dyn;
        hipLaunchKernelGGL(bp_wave_analysis, dim3((unsigned)n), dim3(WAVE_THREADS), lds_bytes(p.M), h->stream, a);
        HIPCHK(hipGetLastError());
    }
    if (dyn) {
        HIPCHK(wave_dnat_launch(h->nat_np, Y, F, c->n_sent, D, (const float *)(din + w.mean), (const float *)(din + w.istd), nat_d, h->stream));
    } else if (nat) {
        HIPCHK(wave_nat_launch(rows_d, F, c->n_sent, D, ctx, toff, nat_d, h->stream));
    }
    window_adopt(h, n, D, ctx, nat, false);
    if ((r = forward_resident(h, n)) != BP_OK) return r;
    HIPCHK(wave_synthesis_launch(h->out_chunk.as<float>(), h->ld[L - 1], c->out_col, Y, win, tw, p.log2M, D, c->target, (float *)h->wave[2].p, n,
                                 h->stream, h->post_on ? &h->post : nullptr));
    hipLaunchKernelGGL(bp_wave_overlap, dim3((unsigned)n), dim3(WAVE_THREADS), 0, h->stream, (const float *)h->wave[2].p, win, F, c->n_sent, p.hop,
                       (float *)h->wave[3].p);
    HIPCHK(hipGetLastError());
    float *hout = (float *)h->wave_pin[1].p;
    HIPCHK(hipMemcpyAsync(hout, h->wave[3].p, pcm_b, hipMemcpyDeviceToHost, h->stream));
    if (out_net && (r = outputs_to_host(h, n)) != BP_OK) return r;
    HIPCHK(hipStreamSynchronize(h->stream));
    wave_gather(out_pcm, p, c->sent_len, hout);
    if (out_net) unpad_rows(out_net, sL, h->host_out.as<float>(), h->ld[L - 1], n);
    return BP_OK;
}
