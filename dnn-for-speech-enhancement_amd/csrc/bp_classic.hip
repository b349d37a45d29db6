// bp_classic.hip -- C-ABI implementation (include/bp_c_api.h), part 8 of 9: the classic baseline.  The log-MMSE (Ephraim-Malah
// log-spectral-amplitude) enhancer on the signal definition of bp_wave.hip: noisy PCM in, enhanced PCM out, no net
// (bp_logmmse_waves here; bp_eval_mix_logmmse in bp_mix.hip through bp_classic.h).  Definition: include/bp_c_api.h,
// INTEGRATION.md 1h.  gfx950 only.
//
// A call is bp_wave_analysis (bp_wave.hip) -> bp_logmmse_gain -> bp_wave_synthesis with BP_WAVE_MASK and the gain rows in place of
// the net's output -> bp_wave_overlap.  The one kernel of this unit:
//   bp_logmmse_gain  one workgroup of 256 threads per sentence; the frames of a sentence are a dependent chain (the noise estimate
//                    and the decision-directed a-priori SNR carry over), the bins are independent but for the VAD, the mean of the
//                    log likelihood ratio over all bins of a frame.  Thread i owns bins i, i + 256, ... (NB of them, 5 at fea_dim
//                    1025): lambda and A_prev stay in double registers, the mean is a shuffle tree per wave64 and one LDS slot per
//                    wave (two sets, alternating: one barrier per frame), and frame t+1's Y is loaded -- unconditionally, from a
//                    clamped row and bin -- before frame t's arithmetic, so that the chain does not wait for memory.  The noise
//                    start (the mean power of the first init_frames frames) is the kernel's prologue.
// No float atomics, one summation order: the same bits on every run, whatever else shares the call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "bp_classic.h"
#include "bp_fft.h"
#include "bp_handle.h"

namespace {

struct LogmmseArgs {
    const float2 *Y; const int *F;
    float *gain, *vad;
    int D, init_frames;
    double alpha, mu, eta, xi_min, gamma_max;
};

}  // namespace

template <int NB>
__global__ __launch_bounds__(WAVE_THREADS) void bp_logmmse_gain(const LogmmseArgs a)
{
    __shared__ double red[2][WAVE_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x, D = a.D, f0 = a.F[s], T = a.F[s + 1] - f0;
    const float2 *Y = a.Y + (size_t)f0 * D;
    float *gain = a.gain + (size_t)f0 * D;
    int kc[NB];                                                  // this thread's bins, clamped: loads need no predicate
    bool on[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) { const int k = tid + j * WAVE_THREADS; on[j] = k < D; kc[j] = on[j] ? k : D - 1; }
    // the noise start
    const int ni = a.init_frames < T ? a.init_frames : T;
    double lam[NB], Ap[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) { lam[j] = 0.0; Ap[j] = 0.0; }
    for (int t = 0; t < ni; ++t) {
#pragma unroll
        for (int j = 0; j < NB; ++j) lam[j] += lm_power(Y[(size_t)t * D + kc[j]]);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) lam[j] = lm_noise_start(lam[j], ni);
    float2 cur[NB], nxt[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) cur[j] = Y[kc[j]];
    for (int t = 0; t < T; ++t) {
        const size_t rn = (size_t)(t + 1 < T ? t + 1 : T - 1) * D;
#pragma unroll
        for (int j = 0; j < NB; ++j) nxt[j] = Y[rn + kc[j]];
        float g[NB];                                             // (the other set of slots is written next: one barrier per frame)
        const double vad = lm_frame<NB>(a.alpha, a.mu, a.eta, a.xi_min, a.gamma_max, D, t == 0, cur, on, lam, Ap, red[t & 1], g);
#pragma unroll
        for (int j = 0; j < NB; ++j) if (on[j]) gain[(size_t)t * D + tid + j * WAVE_THREADS] = g[j];
        if (tid == 0) a.vad[f0 + t] = (float)vad;
#pragma unroll
        for (int j = 0; j < NB; ++j) cur[j] = nxt[j];
    }
}

// ------------------------------------------------------------------ log-MMSE streams: one launch per push
namespace {

// One job per channel that gets output frames in a push: frames t0 .. t0 + nf - 1 of the channel's sentence, frame t0 + i starting
// at hop unit `unit` + i of the block's samples ([carry | new], zeros behind a sentence's end).  t0 == 0: the job holds the frames
// of the noise start (nf >= init_frames, or the whole sentence).  out_n samples go to out_off of the compact output.
struct LmJob { int chan, unit, t0, nf, ended, out_off, out_n, pad; };

struct LmStreamArgs {
    const LmJob *jobs; const float *pcm, *win; const float2 *tw;
    double *lam, *Ap;                       // [n_chan][D]
    float *half;                            // [n_chan][hop]: the second half of the channel's last synthesised frame
    float *out;                             // compact output of the push
    int log2M, D, init_frames;
    double alpha, mu, eta, xi_min, gamma_max;
};

// LDS of bp_lmstream_push, in bytes from the start: synth_frame's FFT space and S | two frames | the Y row | the VAD slots | the gain row
__host__ __device__ inline size_t lm_frames_at(int M) { return (lds_bytes(M) + (size_t)(M + 1) * sizeof(float2) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t lm_yrow_at(int M) { return lm_frames_at(M) + (size_t)4 * M * sizeof(float); }
__host__ __device__ inline size_t lm_red_at(int M) { return lm_yrow_at(M) + (size_t)(M + 1) * sizeof(float2); }
__host__ __device__ inline size_t lm_gain_at(int M) { return lm_red_at(M) + (WAVE_THREADS / 64) * sizeof(double); }
__host__ __device__ inline size_t lm_lds_bytes(int M) { return lm_gain_at(M) + (size_t)(M + 1) * sizeof(float); }

}  // namespace

// One workgroup takes one channel's new frames from PCM to PCM: per frame, serially, the analysis (rfft_frame, rfft_bin), the
// recursion step (lm_frame), the synthesis (synth_frame with BP_WAVE_MASK on the Y row and the gain row, both in LDS) and the
// overlap-add with the frame before it (overlap4) -- the device functions, and so the bits, of the four launches of
// bp_logmmse_waves.  lambda and A_prev stay in registers across the job's frames and in the channel's state between pushes.
template <int NB>
__global__ __launch_bounds__(WAVE_THREADS) void bp_lmstream_push(const LmStreamArgs a)
{
    extern __shared__ __align__(16) float2 lm_lds[];
    const LmJob job = a.jobs[blockIdx.x];
    const int tid = threadIdx.x, D = a.D, M = 1 << a.log2M, hop = M, N = 2 * M;
    char *lds = reinterpret_cast<char *>(lm_lds);
    float2 *z = lm_lds;
    float *fr = reinterpret_cast<float *>(lds + lm_frames_at(M));    // fr[2][N]: frame i of the job in fr[i & 1]
    float2 *Yrow = reinterpret_cast<float2 *>(lds + lm_yrow_at(M));
    double *red = reinterpret_cast<double *>(lds + lm_red_at(M));
    float *grow = reinterpret_cast<float *>(lds + lm_gain_at(M));
    const float *x0 = a.pcm + (size_t)job.unit * hop;
    int kc[NB];                                                  // this thread's bins, clamped
    bool on[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) { const int k = tid + j * WAVE_THREADS; on[j] = k < D; kc[j] = on[j] ? k : D - 1; }
    double lam[NB], Ap[NB];
    if (job.t0 == 0) {
        // the noise start: the mean power of the sentence's first min(init_frames, T) frames (their FFTs are computed again below)
        const int ni = a.init_frames < job.nf ? a.init_frames : job.nf;
#pragma unroll
        for (int j = 0; j < NB; ++j) { lam[j] = 0.0; Ap[j] = 0.0; }
        for (int t = 0; t < ni; ++t) {
            rfft_frame(z, x0 + (size_t)t * hop, a.win, a.tw, a.log2M);
#pragma unroll
            for (int j = 0; j < NB; ++j) lam[j] += lm_power(rfft_bin(z, a.tw, M, kc[j]));
            __syncthreads();                                     // (the next frame is scattered over z)
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) lam[j] = lm_noise_start(lam[j], ni);
    } else {
#pragma unroll
        for (int j = 0; j < NB; ++j) { lam[j] = a.lam[(size_t)job.chan * D + kc[j]]; Ap[j] = a.Ap[(size_t)job.chan * D + kc[j]]; }
        const float *hs = a.half + (size_t)job.chan * hop;      // the frame before the job's first: as the second half of fr[1]
        for (int q = tid; q < hop / 4; q += WAVE_THREADS)
            *reinterpret_cast<float4 *>(fr + N + hop + 4 * q) = *reinterpret_cast<const float4 *>(hs + 4 * q);
    }
    for (int i = 0; i < job.nf; ++i) {
        const int t = job.t0 + i;
        rfft_frame(z, x0 + (size_t)i * hop, a.win, a.tw, a.log2M);
        float2 y[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) { y[j] = rfft_bin(z, a.tw, M, kc[j]); if (on[j]) Yrow[kc[j]] = y[j]; }
        float g[NB];
        (void)lm_frame<NB>(a.alpha, a.mu, a.eta, a.xi_min, a.gamma_max, D, t == 0, y, on, lam, Ap, red, g);
#pragma unroll
        for (int j = 0; j < NB; ++j) if (on[j]) grow[kc[j]] = g[j];
        __syncthreads();
        float *cur = fr + (size_t)(i & 1) * N;
        const float *pv = fr + (size_t)((i & 1) ^ 1) * N + hop;
        synth_frame(z, grow, Yrow, a.win, a.tw, a.log2M, BP_WAVE_MASK, cur);
        __syncthreads();
        if (t > 0) {                                             // frame 0 of a sentence covers the front padding: no output
            const int off = (t - 1 - (job.t0 > 0 ? job.t0 - 1 : 0)) * hop, n = job.out_n - off;   // clipped at a sentence's end
            float *dst = a.out + job.out_off + off;              // compact: only 4-byte aligned
            for (int q = tid; q < hop / 4; q += WAVE_THREADS) {
                const float4 c = *reinterpret_cast<const float4 *>(cur + 4 * q), b = *reinterpret_cast<const float4 *>(pv + 4 * q);
                const float4 wa = *reinterpret_cast<const float4 *>(a.win + 4 * q), wb = *reinterpret_cast<const float4 *>(a.win + hop + 4 * q);
                const float4 r = overlap4(c, b, wa, wb);
                const int e = 4 * q;
                if (e < n) dst[e] = r.x;
                if (e + 1 < n) dst[e + 1] = r.y;
                if (e + 2 < n) dst[e + 2] = r.z;
                if (e + 3 < n) dst[e + 3] = r.w;
            }
        }
    }
    if (!job.ended) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if (on[j]) { a.lam[(size_t)job.chan * D + kc[j]] = lam[j]; a.Ap[(size_t)job.chan * D + kc[j]] = Ap[j]; }
        const float *last = fr + (size_t)((job.nf - 1) & 1) * N + hop;
        float *hd = a.half + (size_t)job.chan * hop;
        for (int q = tid; q < hop / 4; q += WAVE_THREADS)
            *reinterpret_cast<float4 *>(hd + 4 * q) = *reinterpret_cast<const float4 *>(last + 4 * q);
    }
}

// ------------------------------------------------------------------ host side
int logmmse_check(const char *who, const bp_logmmse_params *p, LogmmseP &out)
{
    bp_logmmse_params d;
    bp_logmmse_defaults(&d);
    if (p) d = *p;
    const std::string w(who);
    if (!(d.alpha >= 0.0 && d.alpha < 1.0)) return fail(BP_ERR_ARG, w + ": need 0 <= alpha < 1");
    if (!(d.mu >= 0.0 && d.mu <= 1.0)) return fail(BP_ERR_ARG, w + ": need 0 <= mu <= 1");
    if (!std::isfinite(d.eta)) return fail(BP_ERR_ARG, w + ": eta is not finite");
    if (!(d.xi_min_db >= -100.0 && d.xi_min_db <= 0.0)) return fail(BP_ERR_ARG, w + ": need -100 <= xi_min_db <= 0");
    if (!(d.gamma_max >= 1.0) || !std::isfinite(d.gamma_max)) return fail(BP_ERR_ARG, w + ": need a finite gamma_max >= 1");
    if (d.init_frames < 1) return fail(BP_ERR_ARG, w + ": need init_frames >= 1");
    out.alpha = d.alpha; out.mu = d.mu; out.eta = d.eta; out.xi_min = pow(10.0, d.xi_min_db / 10.0); out.gamma_max = d.gamma_max;
    out.init_frames = d.init_frames;
    return BP_OK;
}

hipError_t logmmse_gain_launch(const LogmmseP &p, const float2 *Y, const int *F, int n_sent, int D, float *gain, float *vad, hipStream_t st)
{
    LogmmseArgs a; memset(&a, 0, sizeof(a));
    a.Y = Y; a.F = F; a.gain = gain; a.vad = vad; a.D = D; a.init_frames = p.init_frames;
    a.alpha = p.alpha; a.mu = p.mu; a.eta = p.eta; a.xi_min = p.xi_min; a.gamma_max = p.gamma_max;
    const dim3 grid((unsigned)n_sent), blk(WAVE_THREADS);
    switch ((D + WAVE_THREADS - 1) / WAVE_THREADS) {             // fea_dim 33 .. 129, 257, 513, 1025
    case 1: hipLaunchKernelGGL(bp_logmmse_gain<1>, grid, blk, 0, st, a); break;
    case 2: hipLaunchKernelGGL(bp_logmmse_gain<2>, grid, blk, 0, st, a); break;
    case 3: hipLaunchKernelGGL(bp_logmmse_gain<3>, grid, blk, 0, st, a); break;
    default: hipLaunchKernelGGL(bp_logmmse_gain<5>, grid, blk, 0, st, a); break;
    }
    return hipGetLastError();
}

extern "C" int bp_logmmse_defaults(bp_logmmse_params *p)
{
    if (!p) return fail(BP_ERR_ARG, "bp_logmmse_defaults: null pointer");
    p->alpha = 0.98; p->mu = 0.98; p->eta = 0.15; p->xi_min_db = -25.0; p->gamma_max = 40.0; p->init_frames = 6;
    return BP_OK;
}

extern "C" int bp_logmmse_waves(int device, int fea_dim, const bp_logmmse_params *p, int n_sent, const int *sent_len, const float *pcm,
                                float *out_pcm, float *out_gain, float *out_vad)
{
    const int log2M = wave_log2_fft(fea_dim);
    if (log2M < 0) return fail(BP_ERR_ARG, "bp_logmmse_waves: 2*(fea_dim-1) must be a power of two from 64 to 2048");
    LogmmseP lp;
    { const int r = logmmse_check("bp_logmmse_waves", p, lp); if (r != BP_OK) return r; }
    if (n_sent < 1 || !sent_len || !pcm || !out_pcm) return fail(BP_ERR_ARG, "bp_logmmse_waves: no sentences or null pointer");
    const int M = 1 << log2M, hop = M, N = 2 * M, D = fea_dim;
    std::vector<int> F((size_t)n_sent + 1, 0);
    size_t f = 0;
    for (int s = 0; s < n_sent; ++s) {
        if (sent_len[s] < 1) return fail(BP_ERR_ARG, "bp_logmmse_waves: empty sentence " + std::to_string(s));
        f += (size_t)((sent_len[s] - 1) / hop + 2);
        if (f > (size_t)INT32_MAX / 8) return fail(BP_ERR_ARG, "bp_logmmse_waves: too many frames in one call");
        F[s + 1] = (int)f;
    }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(BP_ERR_ARG, "bp_logmmse_waves: device ordinal out of range");
    HIPCHK(hipSetDevice(device));
    const auto al256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // one host->device block: F | window | twiddles | padded PCM (the layout of bp_wave_lps: sentence s at sample (F_s + s + 1) hop);
    // one device->host block: padded enhanced PCM | vad | gain; between them the spectrum and the synthesis frames
    const size_t padded = (f + (size_t)n_sent) * hop;
    const size_t o_win = al256(((size_t)n_sent + 1) * 4), o_tw = o_win + al256((size_t)N * 4), o_pcm = o_tw + al256((size_t)(M + 1) * 8);
    const size_t in_b = o_pcm + al256(padded * 4);
    const size_t o_out = in_b, o_vad = o_out + al256(padded * 4), o_gain = o_vad + al256(f * 4), out_end = o_gain + al256(f * D * 4);
    const size_t o_Y = out_end, o_syn = o_Y + al256(f * D * sizeof(float2)), total = o_syn + al256(f * N * 4);
    const size_t out_b = (out_gain ? out_end : out_vad ? o_gain : o_vad) - o_out;
    std::vector<char> hb(in_b, 0), ho(out_b);
    memcpy(hb.data(), F.data(), F.size() * 4);
    wave_window_twiddles(log2M, (float *)(hb.data() + o_win), (float2 *)(hb.data() + o_tw));
    {
        float *x = (float *)(hb.data() + o_pcm);
        size_t src = 0;
        for (int s = 0; s < n_sent; ++s) {
            memcpy(x + (size_t)(F[s] + s + 1) * hop, pcm + src, (size_t)sent_len[s] * 4);
            src += (size_t)sent_len[s];
        }
    }
    hipStream_t st = nullptr;
    char *d = nullptr;
    int rc = BP_OK;
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&d, total);
    if (e == hipSuccess) e = hipMemcpyAsync(d, hb.data(), in_b, hipMemcpyHostToDevice, st);
    const float *win = (const float *)(d + o_win);
    const float2 *tw = (const float2 *)(d + o_tw);
    const int *Fd = (const int *)d;
    float2 *Y = (float2 *)(d + o_Y);
    float *gain = (float *)(d + o_gain), *syn = (float *)(d + o_syn);
    if (e == hipSuccess) {
        WaveAnaArgs a; memset(&a, 0, sizeof(a));
        a.pcm = (const float *)(d + o_pcm); a.win = win; a.tw = tw; a.F = Fd;
        a.n_sent = n_sent; a.log2M = log2M; a.D = D; a.hop = hop; a.ctx = 1;
        a.Y = Y;
        e = wave_analysis_launch(a, (int)f, st);
    }
    if (e == hipSuccess) e = logmmse_gain_launch(lp, Y, Fd, n_sent, D, gain, (float *)(d + o_vad), st);
    if (e == hipSuccess) e = wave_synthesis_launch(gain, D, 0, Y, win, tw, log2M, D, BP_WAVE_MASK, syn, (int)f, st);
    if (e == hipSuccess) e = wave_overlap_launch(syn, win, Fd, n_sent, hop, (float *)(d + o_out), (int)f, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ho.data(), d + o_out, out_b, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = fail(BP_ERR_DEVICE, std::string("bp_logmmse_waves: ") + hipGetErrorString(e));
    if (d) (void)hipFree(d);
    if (st) (void)hipStreamDestroy(st);
    if (rc != BP_OK) return rc;
    const float *xo = (const float *)ho.data();
    size_t dst = 0;
    for (int s = 0; s < n_sent; ++s) {
        memcpy(out_pcm + dst, xo + (size_t)(F[s] + s + 1) * hop, (size_t)sent_len[s] * 4);
        dst += (size_t)sent_len[s];
    }
    if (out_vad) memcpy(out_vad, ho.data() + (o_vad - o_out), f * 4);
    if (out_gain) memcpy(out_gain, ho.data() + (o_gain - o_out), f * D * 4);
    return BP_OK;
}

// ------------------------------------------------------------------ log-MMSE streams: host side
namespace {

// What a channel has produced after `received` samples of its sentence (include/bp_c_api.h): bp_stream_counts with look-ahead 0
// and the noise start in place of the noise-aware row
struct LmCounts { int64_t fi, fo, so; };
LmCounts lm_counts(int hop, int init_frames, int64_t received, bool ended)
{
    LmCounts c = {0, 0, 0};
    if (received <= 0) return c;
    const int64_t T = (received - 1) / hop + 2;
    c.fi = ended ? T : received / hop;
    const bool known = ended || c.fi >= init_frames;
    c.fo = !known ? 0 : c.fi;
    c.so = ended ? received : std::max<int64_t>(0, c.fo - 1) * hop;
    return c;
}

// The carry holds the padded samples from the channel's first frame without output on: hop zeros in front of a sentence, all of
// the sentence while it waits for its noise start, the last hop + received % hop samples after that.
struct LmChan { int64_t received; size_t carry_n; std::vector<float> carry; };
struct LmPlan { int64_t r1; bool ended; LmCounts c0, c1; };

size_t lm_al256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

struct bp_lmstream {
    int device, D, hop, log2M, n_chan, max_push;
    LogmmseP lp;
    hipStream_t st;
    std::vector<LmChan> ch;
    std::vector<LmPlan> plan;
    std::vector<LmJob> jobs;
    size_t max_units;            // hop units of samples in one push's input block at most (and of its output)
    char *dev;                   // window | twiddles | lambda | A_prev | half frames | input block | output samples
    size_t o_win, o_tw, o_lam, o_Ap, o_half, o_in, o_out, o_pcm;   // o_pcm: the samples' place in the input block, behind n_chan jobs
    char *pin_in; float *pin_out;
};

static void lmstream_release(bp_lmstream *s)
{
    if (s->dev) (void)hipFree(s->dev);
    if (s->pin_in) (void)hipHostFree(s->pin_in);
    if (s->pin_out) (void)hipHostFree(s->pin_out);
    if (s->st) (void)hipStreamDestroy(s->st);
    delete s;
}

extern "C" int bp_lmstream_counts(int fea_dim, int init_frames, int64_t received, int ended, int64_t *frames_in, int64_t *frames_out,
                                  int64_t *samples_out)
{
    if (wave_log2_fft(fea_dim) < 0) return fail(BP_ERR_ARG, "bp_lmstream_counts: 2*(fea_dim-1) must be a power of two from 64 to 2048");
    if (init_frames < 1) return fail(BP_ERR_ARG, "bp_lmstream_counts: need init_frames >= 1");
    if (received < 0) return fail(BP_ERR_ARG, "bp_lmstream_counts: received < 0");
    if (!frames_in || !frames_out || !samples_out) return fail(BP_ERR_ARG, "bp_lmstream_counts: null output");
    const LmCounts c = lm_counts(fea_dim - 1, init_frames, received, ended != 0);
    *frames_in = c.fi; *frames_out = c.fo; *samples_out = c.so;
    return BP_OK;
}

extern "C" int bp_lmstream_open(int device, int fea_dim, const bp_logmmse_params *p, int n_chan, int max_push_samples, bp_lmstream **out)
{
    const int log2M = wave_log2_fft(fea_dim);
    if (log2M < 0) return fail(BP_ERR_ARG, "bp_lmstream_open: 2*(fea_dim-1) must be a power of two from 64 to 2048");
    LogmmseP lp;
    { const int r = logmmse_check("bp_lmstream_open", p, lp); if (r != BP_OK) return r; }
    if (n_chan < 1 || n_chan > (1 << 16)) return fail(BP_ERR_ARG, "bp_lmstream_open: n_chan must be in 1 .. 65536");
    if (max_push_samples < 1) return fail(BP_ERR_ARG, "bp_lmstream_open: max_push_samples must be >= 1");
    if (!out) return fail(BP_ERR_ARG, "bp_lmstream_open: null pointer");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(BP_ERR_ARG, "bp_lmstream_open: device ordinal out of range");
    HIPCHK(hipSetDevice(device));
    const int D = fea_dim, hop = D - 1, N = 2 * hop, nc = n_chan;
    int lds_max = 0;
    HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    if (lm_lds_bytes(hop) > (size_t)lds_max)
        return fail(BP_ERR_DEVICE, "bp_lmstream_open: the kernel needs " + std::to_string(lm_lds_bytes(hop)) + " bytes of LDS, the device has " +
                                   std::to_string(lds_max) + " per workgroup");

    bp_lmstream *s = new (std::nothrow) bp_lmstream();
    if (!s) return fail(BP_ERR_NOMEM, "bp_lmstream_open: out of memory");
    s->device = device; s->D = D; s->hop = hop; s->log2M = log2M; s->n_chan = nc; s->max_push = max_push_samples; s->lp = lp;
    s->st = nullptr; s->dev = nullptr; s->pin_in = nullptr; s->pin_out = nullptr;
    // A channel's job holds what waited -- fewer than init_frames hops of samples behind the hop of front padding -- and what
    // arrived, rounded up to frames, plus the two frames an end adds and the hop behind the last frame's start:
    // at most init_frames + n_in / hop + 4 hop units.
    s->max_units = (size_t)nc * ((size_t)lp.init_frames + 4) + (size_t)max_push_samples / hop;
    const size_t carry_cap = ((size_t)lp.init_frames + 2) * hop;
    if (s->max_units * hop > (size_t)INT32_MAX) { lmstream_release(s); return fail(BP_ERR_NOMEM, "bp_lmstream_open: the blocks of a push would exceed 2^31 samples"); }
    size_t o = 0;
    s->o_win = o; o += lm_al256((size_t)N * 4);
    s->o_tw = o; o += lm_al256((size_t)(hop + 1) * 8);
    const size_t consts = o;
    s->o_lam = o; o += lm_al256((size_t)nc * D * 8);
    s->o_Ap = o; o += lm_al256((size_t)nc * D * 8);
    s->o_half = o; o += lm_al256((size_t)nc * hop * 4);
    const size_t state_end = o;
    s->o_pcm = lm_al256((size_t)nc * sizeof(LmJob));
    const size_t in_cap = s->o_pcm + lm_al256(s->max_units * hop * 4), out_cap = lm_al256(s->max_units * hop * 4);
    s->o_in = o; o += in_cap;
    s->o_out = o; o += out_cap;
    hipError_t e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e != hipSuccess) { lmstream_release(s); return fail(BP_ERR_DEVICE, std::string("bp_lmstream_open: ") + hipGetErrorString(e)); }
    e = hipMalloc((void **)&s->dev, o);
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->pin_in, std::max(in_cap, consts));
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->pin_out, out_cap);
    bool host_ok = e == hipSuccess;
    if (host_ok) {
        try {
            s->ch.resize(nc);
            for (LmChan &ch : s->ch) { ch.received = 0; ch.carry_n = hop; ch.carry.assign(carry_cap, 0.0f); }
            s->plan.resize(nc);
            s->jobs.reserve(nc);
        } catch (const std::bad_alloc &) { host_ok = false; }
    }
    if (!host_ok) {
        (void)hipGetLastError();
        lmstream_release(s);
        return fail(BP_ERR_NOMEM, std::string("bp_lmstream_open: ") + (e != hipSuccess ? hipGetErrorString(e) : "out of host memory"));
    }
    // constants, once: window and twiddles (computed in double and rounded once, as bp_logmmse_waves does)
    memset(s->pin_in, 0, consts);
    wave_window_twiddles(log2M, (float *)(s->pin_in + s->o_win), (float2 *)(s->pin_in + s->o_tw));
    e = hipMemcpyAsync(s->dev, s->pin_in, consts, hipMemcpyHostToDevice, s->st);
    if (e == hipSuccess) e = hipMemsetAsync(s->dev + consts, 0, state_end - consts, s->st);
    if (e == hipSuccess) e = hipStreamSynchronize(s->st);
    if (e != hipSuccess) { lmstream_release(s); return fail(BP_ERR_DEVICE, std::string("bp_lmstream_open: ") + hipGetErrorString(e)); }
    *out = s;
    return BP_OK;
}

extern "C" int bp_lmstream_close(bp_lmstream *s)
{
    if (!s) return BP_OK;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->st);
    lmstream_release(s);
    return BP_OK;
}

extern "C" int bp_lmstream_push(bp_lmstream *s, const int *n_in, const float *pcm, const unsigned char *end, int *n_out, float *out_pcm,
                                size_t out_cap)
{
    if (!s || !n_in || !n_out) return fail(BP_ERR_ARG, "bp_lmstream_push: null argument");
    const int D = s->D, hop = s->hop, nc = s->n_chan, init = s->lp.init_frames;
    // ---- the plan: counts before and after, per channel (nothing of the stream changes until every check has passed)
    int64_t total_in = 0, due = 0, units = 0;
    for (int c = 0; c < nc; ++c) {
        if (n_in[c] < 0) return fail(BP_ERR_ARG, "bp_lmstream_push: n_in[" + std::to_string(c) + "] < 0");
        total_in += n_in[c];
        if (total_in > s->max_push)
            return fail(BP_ERR_ARG, "bp_lmstream_push: more than max_push_samples = " + std::to_string(s->max_push) + " samples in one push");
    }
    if (total_in > 0 && !pcm) return fail(BP_ERR_ARG, "bp_lmstream_push: null pcm");
    for (int c = 0; c < nc; ++c) {
        LmPlan &p = s->plan[c];
        const LmChan &ch = s->ch[c];
        p.r1 = ch.received + n_in[c];
        p.ended = end && end[c] && p.r1 > 0;
        p.c0 = lm_counts(hop, init, ch.received, false);
        p.c1 = lm_counts(hop, init, p.r1, p.ended);
        due += p.c1.so - p.c0.so;
        if (p.c1.fo > p.c0.fo) units += p.c1.fo - p.c0.fo + 1;
    }
    if ((size_t)due > out_cap) return fail(BP_ERR_ARG, "bp_lmstream_push: " + std::to_string(due) + " samples are due, out_cap is " + std::to_string(out_cap));
    if (due > 0 && !out_pcm) return fail(BP_ERR_ARG, "bp_lmstream_push: null out_pcm");
    if ((size_t)units > s->max_units || (size_t)due > s->max_units * hop)
        return fail(BP_ERR_STATE, "bp_lmstream_push: internal: more frames than the stream was sized for");
    // ---- the input block: one job per channel with output frames | their [carry | new] samples at hop-aligned places (the pinned
    // block is reused by every push: the previous one ended in a synchronisation); with it the channels' new carry
    s->jobs.clear();
    float *hp = (float *)(s->pin_in + s->o_pcm);
    size_t unit = 0, src = 0;
    int64_t out_base = 0;
    for (int c = 0; c < nc; ++c) {
        const LmPlan &p = s->plan[c];
        LmChan &ch = s->ch[c];
        const float *in = pcm ? pcm + src : nullptr;
        const size_t n = (size_t)n_in[c];
        src += n;
        const int64_t fo0 = p.c0.fo, fo1 = p.c1.fo, nf = fo1 - fo0;
        n_out[c] = (int)(p.c1.so - p.c0.so);
        if (nf > 0) {
            // frame fo0 + i starts at unit + i; zeros behind a sentence's end
            float *x = hp + unit * hop;
            const size_t seg = (size_t)(nf + 1) * hop, nca = std::min(seg, ch.carry_n), nin = std::min(seg - nca, n);
            memcpy(x, ch.carry.data(), nca * 4);
            if (nin) memcpy(x + nca, in, nin * 4);
            memset(x + nca + nin, 0, (seg - nca - nin) * 4);
            LmJob j; memset(&j, 0, sizeof(j));
            j.chan = c; j.unit = (int)unit; j.t0 = (int)fo0; j.nf = (int)nf; j.ended = p.ended ? 1 : 0;
            j.out_off = (int)out_base; j.out_n = n_out[c];
            s->jobs.push_back(j);
            unit += (size_t)(nf + 1);
            out_base += n_out[c];
        }
        // the carry: a new sentence starts from hop zeros; else the last hop + r1 - fo1 hop samples of [carry | new]
        if (p.ended) { ch.received = 0; ch.carry_n = hop; memset(ch.carry.data(), 0, (size_t)hop * 4); }
        else if (n > 0) {
            const size_t keep = (size_t)hop + (size_t)(p.r1 - fo1 * hop);
            if (n >= keep) memcpy(ch.carry.data(), in + (n - keep), keep * 4);
            else {
                const size_t old = keep - n;                        // (old <= carry_n: carry_n + n >= keep)
                memmove(ch.carry.data(), ch.carry.data() + (ch.carry_n - old), old * 4);
                memcpy(ch.carry.data() + old, in, n * 4);
            }
            ch.carry_n = keep; ch.received = p.r1;
        }
    }
    if (s->jobs.empty()) return BP_OK;                              // no channel got a new output frame: no device work
    HIPCHK(hipSetDevice(s->device));
    memcpy(s->pin_in, s->jobs.data(), s->jobs.size() * sizeof(LmJob));
    char *din = s->dev + s->o_in;
    HIPCHK(hipMemcpyAsync(din, s->pin_in, s->o_pcm + unit * hop * 4, hipMemcpyHostToDevice, s->st));
    LmStreamArgs a; memset(&a, 0, sizeof(a));
    a.jobs = (const LmJob *)din; a.pcm = (const float *)(din + s->o_pcm);
    a.win = (const float *)(s->dev + s->o_win); a.tw = (const float2 *)(s->dev + s->o_tw);
    a.lam = (double *)(s->dev + s->o_lam); a.Ap = (double *)(s->dev + s->o_Ap); a.half = (float *)(s->dev + s->o_half);
    a.out = (float *)(s->dev + s->o_out);
    a.log2M = s->log2M; a.D = D; a.init_frames = init;
    a.alpha = s->lp.alpha; a.mu = s->lp.mu; a.eta = s->lp.eta; a.xi_min = s->lp.xi_min; a.gamma_max = s->lp.gamma_max;
    const dim3 grid((unsigned)s->jobs.size()), blk(WAVE_THREADS);
    const size_t lds = lm_lds_bytes(hop);
    switch ((D + WAVE_THREADS - 1) / WAVE_THREADS) {                // fea_dim 33 .. 129, 257, 513, 1025
    case 1: hipLaunchKernelGGL(bp_lmstream_push<1>, grid, blk, lds, s->st, a); break;
    case 2: hipLaunchKernelGGL(bp_lmstream_push<2>, grid, blk, lds, s->st, a); break;
    case 3: hipLaunchKernelGGL(bp_lmstream_push<3>, grid, blk, lds, s->st, a); break;
    default: hipLaunchKernelGGL(bp_lmstream_push<5>, grid, blk, lds, s->st, a); break;
    }
    HIPCHK(hipGetLastError());
    if (due > 0) HIPCHK(hipMemcpyAsync(s->pin_out, s->dev + s->o_out, (size_t)due * 4, hipMemcpyDeviceToHost, s->st));
    HIPCHK(hipStreamSynchronize(s->st));
    if (due > 0) memcpy(out_pcm, s->pin_out, (size_t)due * 4);
    return BP_OK;
}
