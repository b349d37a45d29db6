// bp_classic.hip -- C-ABI implementation (include/bp_c_api.h): the classic baseline.  The log-MMSE (Ephraim-Malah
// log-spectral-amplitude) enhancer on the signal definition of bp_wave.hip: noisy PCM in, enhanced PCM out, no net
// (bp_logmmse_waves[_nt] here; bp_eval_mix_logmmse[_nt] in bp_mix.hip through bp_classic.h).  Definition: include/bp_c_api.h,
// INTEGRATION.md 1h, and 1n for the noise tracker of the _nt calls (a second instantiation of both kernels: lm_frame<NB, true>).  gfx950 only.  The second half of the unit is the baseline on live audio (bp_lmstream_*):
// its own job table and kernel; counts, carry, push checks and the owner of its blocks are bp_stream_core.h's, shared with bp_stream.hip.
//
// A call is bp_wave_analysis (bp_wave.hip) -> bp_logmmse_gain -> bp_wave_synthesis with BP_WAVE_MASK and the gain rows in place of
// the net's output -> bp_wave_overlap, on the frame plan and input block of bp_wave_lps (bp_fft.h).  Its kernel:
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
#include <type_traits>
#include <vector>

#include "bp_classic.h"
#include "bp_fft.h"
#include "bp_handle.h"
#include "bp_stream_core.h"

namespace {

// f(std::integral_constant<int, NB>, std::integral_constant<bool, SPP>) for the NB = bins per thread of fea_dim D: 33 .. 129, 257,
// 513, 1025, and the noise update: VAD-gated or the tracker
template <class F> void with_nb(int D, bool spp, F f)
{
    auto g = [&](auto nb) { if (spp) f(nb, std::true_type()); else f(nb, std::false_type()); };
    switch ((D + WAVE_THREADS - 1) / WAVE_THREADS) {
    case 1: g(std::integral_constant<int, 1>()); break;
    case 2: g(std::integral_constant<int, 2>()); break;
    case 3: g(std::integral_constant<int, 3>()); break;
    default: g(std::integral_constant<int, 5>()); break;
    }
}

struct LogmmseArgs {
    const float2 *Y; const int *F;
    float *gain, *vad, *noise;              // noise: null or [frames][D]
    int D, init_frames;
    double alpha, mu, eta, xi_min, gamma_max;
    NoiseP np;
};

}  // namespace

template <int NB, bool SPP>
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
    double lam[NB], Ap[NB], pb[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) { lam[j] = 0.0; Ap[j] = 0.0; pb[j] = 0.0; }
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
        float g[NB], nz[NB];                                     // (the other set of slots is written next: one barrier per frame)
        const double vad = lm_frame<NB, SPP>(a.alpha, a.mu, a.eta, a.xi_min, a.gamma_max, a.np, D, t == 0, cur, on, lam, Ap, pb, red[t & 1], g, nz);
#pragma unroll
        for (int j = 0; j < NB; ++j) if (on[j]) gain[(size_t)t * D + tid + j * WAVE_THREADS] = g[j];
        if (a.noise) {
#pragma unroll
            for (int j = 0; j < NB; ++j) if (on[j]) a.noise[((size_t)f0 + t) * D + tid + j * WAVE_THREADS] = nz[j];
        }
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
    double *pb;                             // [n_chan][D], the tracker's smoothed presence probability; null without the tracker
    float *half;                            // [n_chan][hop]: the second half of the channel's last synthesised frame
    float *out;                             // compact output of the push
    int log2M, D, init_frames;
    double alpha, mu, eta, xi_min, gamma_max;
    NoiseP np;
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
// bp_logmmse_waves.  lambda and A_prev (and the tracker's pbar) stay in registers across the job's frames and in the channel's
// state between pushes.
template <int NB, bool SPP>
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
    double lam[NB], Ap[NB], pb[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) pb[j] = 0.0;                    // (a sentence starts it at 0)
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
        if (SPP) {
#pragma unroll
            for (int j = 0; j < NB; ++j) pb[j] = a.pb[(size_t)job.chan * D + kc[j]];
        }
        copy_half(fr + N + hop, a.half + (size_t)job.chan * hop, hop, WAVE_THREADS);   // the frame before the job's first: as the second half of fr[1]
    }
    for (int i = 0; i < job.nf; ++i) {
        const int t = job.t0 + i;
        rfft_frame(z, x0 + (size_t)i * hop, a.win, a.tw, a.log2M);
        float2 y[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) { y[j] = rfft_bin(z, a.tw, M, kc[j]); if (on[j]) Yrow[kc[j]] = y[j]; }
        float g[NB], nz[NB];
        (void)lm_frame<NB, SPP>(a.alpha, a.mu, a.eta, a.xi_min, a.gamma_max, a.np, D, t == 0, y, on, lam, Ap, pb, red, g, nz);
#pragma unroll
        for (int j = 0; j < NB; ++j) if (on[j]) grow[kc[j]] = g[j];
        __syncthreads();
        float *cur = fr + (size_t)(i & 1) * N;
        const float *pv = fr + (size_t)((i & 1) ^ 1) * N + hop;
        synth_frame(z, grow, Yrow, a.win, a.tw, a.log2M, BP_WAVE_MASK, cur);
        __syncthreads();
        if (t > 0) {                                             // frame 0 of a sentence covers the front padding: no output
            const int off = (t - 1 - (job.t0 > 0 ? job.t0 - 1 : 0)) * hop;
            overlap_store(cur, pv, a.win, hop, a.out + job.out_off + off, job.out_n - off, WAVE_THREADS);   // clipped at a sentence's end
        }
    }
    if (!job.ended) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if (on[j]) { a.lam[(size_t)job.chan * D + kc[j]] = lam[j]; a.Ap[(size_t)job.chan * D + kc[j]] = Ap[j]; }
        if (SPP) {
#pragma unroll
            for (int j = 0; j < NB; ++j) if (on[j]) a.pb[(size_t)job.chan * D + kc[j]] = pb[j];
        }
        copy_half(a.half + (size_t)job.chan * hop, fr + (size_t)((job.nf - 1) & 1) * N + hop, hop, WAVE_THREADS);
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

int noise_check(const char *who, const bp_noise_params *np, NoiseP &out)
{
    bp_noise_params d;
    bp_noise_defaults(&d);
    if (np) d = *np;
    const std::string w(who);
    if (d.mode != BP_NOISE_VAD && d.mode != BP_NOISE_SPP) return fail(BP_ERR_ARG, w + ": noise mode must be BP_NOISE_VAD or BP_NOISE_SPP");
    if (!(d.xi_h1_db >= 0.0 && d.xi_h1_db <= 40.0)) return fail(BP_ERR_ARG, w + ": need 0 <= xi_h1_db <= 40");
    if (!(d.q > 0.0 && d.q < 1.0)) return fail(BP_ERR_ARG, w + ": need 0 < q < 1");
    if (!(d.a_pow >= 0.0 && d.a_pow < 1.0)) return fail(BP_ERR_ARG, w + ": need 0 <= a_pow < 1");
    if (!(d.a_spp >= 0.0 && d.a_spp < 1.0)) return fail(BP_ERR_ARG, w + ": need 0 <= a_spp < 1");
    if (!(d.p_lo > 0.0 && d.p_lo < d.p_cap && d.p_cap < 1.0)) return fail(BP_ERR_ARG, w + ": need 0 < p_lo < p_cap < 1");
    const double xi = pow(10.0, d.xi_h1_db / 10.0);
    out.spp = d.mode == BP_NOISE_SPP;
    out.c0 = (1.0 - d.q) / d.q * (1.0 + xi); out.c1 = xi / (1.0 + xi);
    out.a_pow = d.a_pow; out.a_spp = d.a_spp; out.p_lo = d.p_lo; out.p_cap = d.p_cap;
    return BP_OK;
}

hipError_t logmmse_gain_launch(const LogmmseP &p, const NoiseP &np, const float2 *Y, const int *F, int n_sent, int D, float *gain, float *vad,
                               float *noise, hipStream_t st)
{
    LogmmseArgs a; memset(&a, 0, sizeof(a));
    a.Y = Y; a.F = F; a.gain = gain; a.vad = vad; a.noise = noise; a.D = D; a.init_frames = p.init_frames;
    a.alpha = p.alpha; a.mu = p.mu; a.eta = p.eta; a.xi_min = p.xi_min; a.gamma_max = p.gamma_max; a.np = np;
    const dim3 grid((unsigned)n_sent), blk(WAVE_THREADS);
    with_nb(D, np.spp, [&](auto nb, auto spp) { hipLaunchKernelGGL((bp_logmmse_gain<decltype(nb)::value, decltype(spp)::value>), grid, blk, 0, st, a); });
    return hipGetLastError();
}

extern "C" int bp_noise_defaults(bp_noise_params *p)
{
    if (!p) return fail(BP_ERR_ARG, "bp_noise_defaults: null pointer");
    p->mode = BP_NOISE_SPP; p->xi_h1_db = 15.0; p->q = 0.5; p->a_pow = 0.8; p->a_spp = 0.9; p->p_lo = 0.98; p->p_cap = 0.99;
    return BP_OK;
}

extern "C" int bp_logmmse_defaults(bp_logmmse_params *p)
{
    if (!p) return fail(BP_ERR_ARG, "bp_logmmse_defaults: null pointer");
    p->alpha = 0.98; p->mu = 0.98; p->eta = 0.15; p->xi_min_db = -25.0; p->gamma_max = 40.0; p->init_frames = 6;
    return BP_OK;
}

// bp_logmmse_waves (nt false: the VAD-gated update whatever np, no out_noise) and bp_logmmse_waves_nt
static int logmmse_waves(const char *who, int device, int fea_dim, const bp_logmmse_params *p, bool nt, const bp_noise_params *np,
                         int n_sent, const int *sent_len, const float *pcm, float *out_pcm, float *out_gain, float *out_vad, float *out_noise)
{
    if (wave_log2_fft(fea_dim) < 0) return fail(BP_ERR_ARG, std::string(who) + ": 2*(fea_dim-1) must be a power of two from 64 to 2048");
    LogmmseP lp;
    NoiseP nn = noise_vad();
    { const int r = logmmse_check(who, p, lp); if (r != BP_OK) return r; }
    if (nt) { const int r = noise_check(who, np, nn); if (r != BP_OK) return r; }
    if (!out_pcm) return fail(BP_ERR_ARG, std::string(who) + ": no sentences or null pointer");
    WavePlan wp;
    { const int r = plan_waves(who, fea_dim, n_sent, sent_len, pcm, (size_t)INT32_MAX / 8, wp); if (r != BP_OK) return r; }
    const int D = fea_dim;
    const size_t f = wp.frames;
    // one host->device block, that of bp_wave_lps (no norm file); one device->host block: padded enhanced PCM | vad | gain | noise;
    // between them the spectrum and the synthesis frames
    const WaveIn w = wave_in_layout(wp, D);
    Layout lay(w.bytes);
    const size_t o_out = lay.take(wp.padded * 4), o_vad = lay.take(f * 4), o_gain = lay.take(f * D * 4), o_noise = lay.take(out_noise ? f * D * 4 : 0);
    const size_t out_end = lay.size();
    const size_t o_Y = lay.take(f * D * sizeof(float2)), o_syn = lay.take(f * wp.N * 4), total = lay.size();
    const size_t out_b = (out_noise ? out_end : out_gain ? o_noise : out_vad ? o_gain : o_vad) - o_out;
    OneShot os;
    { const int r = os.open(who, device, total); if (r != BP_OK) return r; }
    std::vector<char> hb(w.bytes), ho(out_b);
    wave_in_fill(hb.data(), w, wp, D, nullptr, nullptr, sent_len, pcm);
    hipError_t &e = os.e;
    char *d = os.d.as<char>();
    if (e == hipSuccess) e = hipMemcpyAsync(d, hb.data(), w.bytes, hipMemcpyHostToDevice, os.st);
    const float *win = (const float *)(d + w.win);
    const float2 *tw = (const float2 *)(d + w.tw);
    const int *Fd = (const int *)(d + w.F);
    float2 *Y = (float2 *)(d + o_Y);
    float *gain = (float *)(d + o_gain), *syn = (float *)(d + o_syn);
    if (e == hipSuccess) {
        WaveAnaArgs a; memset(&a, 0, sizeof(a));
        a.pcm = (const float *)(d + w.pcm); a.win = win; a.tw = tw; a.F = Fd;
        a.n_sent = n_sent; a.log2M = wp.log2M; a.D = D; a.hop = wp.hop; a.ctx = 1;
        a.Y = Y;
        e = wave_analysis_launch(a, (int)f, os.st);
    }
    if (e == hipSuccess) e = logmmse_gain_launch(lp, nn, Y, Fd, n_sent, D, gain, (float *)(d + o_vad), out_noise ? (float *)(d + o_noise) : nullptr, os.st);
    if (e == hipSuccess) e = wave_synthesis_launch(gain, D, 0, Y, win, tw, wp.log2M, D, BP_WAVE_MASK, syn, (int)f, os.st);
    if (e == hipSuccess) e = wave_overlap_launch(syn, win, Fd, n_sent, wp.hop, (float *)(d + o_out), (int)f, os.st);
    if (e == hipSuccess) e = hipMemcpyAsync(ho.data(), d + o_out, out_b, hipMemcpyDeviceToHost, os.st);
    { const int r = os.finish(who); if (r != BP_OK) return r; }
    wave_gather(out_pcm, wp, sent_len, (const float *)ho.data());
    if (out_vad) memcpy(out_vad, ho.data() + (o_vad - o_out), f * 4);
    if (out_gain) memcpy(out_gain, ho.data() + (o_gain - o_out), f * D * 4);
    if (out_noise) memcpy(out_noise, ho.data() + (o_noise - o_out), f * D * 4);
    return BP_OK;
}

extern "C" int bp_logmmse_waves(int device, int fea_dim, const bp_logmmse_params *p, int n_sent, const int *sent_len, const float *pcm,
                                float *out_pcm, float *out_gain, float *out_vad)
{
    return logmmse_waves("bp_logmmse_waves", device, fea_dim, p, false, nullptr, n_sent, sent_len, pcm, out_pcm, out_gain, out_vad, nullptr);
}

extern "C" int bp_logmmse_waves_nt(int device, int fea_dim, const bp_logmmse_params *p, const bp_noise_params *np, int n_sent,
                                   const int *sent_len, const float *pcm, float *out_pcm, float *out_gain, float *out_vad, float *out_noise)
{
    return logmmse_waves("bp_logmmse_waves_nt", device, fea_dim, p, true, np, n_sent, sent_len, pcm, out_pcm, out_gain, out_vad, out_noise);
}

// ------------------------------------------------------------------ log-MMSE streams: host side
struct bp_lmstream {
    int device, D, hop, log2M, n_chan, max_push;
    LogmmseP lp;
    NoiseP np;
    hipStream_t st;
    // a channel's carry holds the padded samples from its first frame without output on: hop zeros in front of a sentence, all
    // of the sentence while it waits for its noise start, the last hop + received % hop samples after that
    std::vector<Carry> ch;
    std::vector<ChanStep> plan;
    std::vector<LmJob> jobs;
    size_t max_units;            // hop units of samples in one push's input block at most (and of its output)
    StreamBlocks blk;            // device: window | twiddles | lambda | A_prev | pbar (tracker) | half frames | input block | output samples
    size_t o_win, o_tw, o_lam, o_Ap, o_pb, o_half, o_in, o_out, o_pcm;   // o_pcm: the samples' place in the input block, behind n_chan jobs
};

static void lmstream_release(bp_lmstream *s)
{
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
    const Counts c = stream_counts(fea_dim - 1, 0, init_frames, received, ended != 0);
    *frames_in = c.fi; *frames_out = c.fo; *samples_out = c.so;
    return BP_OK;
}

// bp_lmstream_open (nt false: the VAD-gated update whatever np) and bp_lmstream_open_nt
static int lmstream_open(const std::string &who, int device, int fea_dim, const bp_logmmse_params *p, bool nt, const bp_noise_params *np,
                         int n_chan, int max_push_samples, bp_lmstream **out)
{
    const int log2M = wave_log2_fft(fea_dim);
    if (log2M < 0) return fail(BP_ERR_ARG, who + ": 2*(fea_dim-1) must be a power of two from 64 to 2048");
    LogmmseP lp;
    NoiseP nn = noise_vad();
    { const int r = logmmse_check(who.c_str(), p, lp); if (r != BP_OK) return r; }
    if (nt) { const int r = noise_check(who.c_str(), np, nn); if (r != BP_OK) return r; }
    if (n_chan < 1 || n_chan > (1 << 16)) return fail(BP_ERR_ARG, who + ": n_chan must be in 1 .. 65536");
    if (max_push_samples < 1) return fail(BP_ERR_ARG, who + ": max_push_samples must be >= 1");
    if (!out) return fail(BP_ERR_ARG, who + ": null pointer");
    { const int r = use_device(who.c_str(), device); if (r != BP_OK) return r; }
    const int D = fea_dim, hop = D - 1, N = 2 * hop, nc = n_chan;
    int lds_max = 0;
    HIPCHK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    if (lm_lds_bytes(hop) > (size_t)lds_max)
        return fail(BP_ERR_DEVICE, who + ": the kernel needs " + std::to_string(lm_lds_bytes(hop)) + " bytes of LDS, the device has " +
                                   std::to_string(lds_max) + " per workgroup");

    bp_lmstream *s = new (std::nothrow) bp_lmstream();
    if (!s) return fail(BP_ERR_NOMEM, who + ": out of memory");
    s->device = device; s->D = D; s->hop = hop; s->log2M = log2M; s->n_chan = nc; s->max_push = max_push_samples; s->lp = lp; s->np = nn;
    // A channel's job holds what waited -- fewer than init_frames hops of samples behind the hop of front padding -- and what
    // arrived, rounded up to frames, plus the two frames an end adds and the hop behind the last frame's start:
    // at most init_frames + n_in / hop + 4 hop units.
    s->max_units = (size_t)nc * ((size_t)lp.init_frames + 4) + (size_t)max_push_samples / hop;
    const size_t carry_cap = ((size_t)lp.init_frames + 2) * hop;
    if (s->max_units * hop > (size_t)INT32_MAX) { lmstream_release(s); return fail(BP_ERR_NOMEM, who + ": the blocks of a push would exceed 2^31 samples"); }
    Layout lay;
    s->o_win = lay.take((size_t)N * 4);
    s->o_tw = lay.take((size_t)(hop + 1) * 8);
    const size_t consts = lay.size();
    s->o_lam = lay.take((size_t)nc * D * 8);
    s->o_Ap = lay.take((size_t)nc * D * 8);
    s->o_pb = lay.take(nn.spp ? (size_t)nc * D * 8 : 0);
    s->o_half = lay.take((size_t)nc * hop * 4);
    const size_t state_end = lay.size();
    Layout in;                                                   // a push's input block: n_chan jobs | samples
    in.take((size_t)nc * sizeof(LmJob));
    s->o_pcm = in.take(s->max_units * hop * 4);
    const size_t in_cap = in.size(), out_cap = al256(s->max_units * hop * 4);
    s->o_in = lay.take(in_cap);
    s->o_out = lay.take(out_cap);
    const size_t o = lay.size();
    hipError_t e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e != hipSuccess) { lmstream_release(s); return fail(BP_ERR_DEVICE, who + ": " + hipGetErrorString(e)); }
    e = s->blk.alloc(o, std::max(in_cap, consts), out_cap);
    bool host_ok = e == hipSuccess;
    if (host_ok) {
        try {
            s->ch.assign(nc, Carry(carry_cap, hop));
            s->plan.resize(nc);
            s->jobs.reserve(nc);
        } catch (const std::bad_alloc &) { host_ok = false; }
    }
    if (!host_ok) {
        (void)hipGetLastError();
        lmstream_release(s);
        return fail(BP_ERR_NOMEM, who + ": " + (e != hipSuccess ? hipGetErrorString(e) : "out of host memory"));
    }
    // constants, once: window and twiddles (computed in double and rounded once, as bp_logmmse_waves does)
    char *pin = s->blk.pin_in.as<char>();
    memset(pin, 0, consts);
    wave_window_twiddles(log2M, (float *)(pin + s->o_win), (float2 *)(pin + s->o_tw));
    e = s->blk.upload_consts(consts, state_end, s->st);
    if (e != hipSuccess) { lmstream_release(s); return fail(BP_ERR_DEVICE, who + ": " + hipGetErrorString(e)); }
    *out = s;
    return BP_OK;
}

extern "C" int bp_lmstream_open(int device, int fea_dim, const bp_logmmse_params *p, int n_chan, int max_push_samples, bp_lmstream **out)
{
    return lmstream_open("bp_lmstream_open", device, fea_dim, p, false, nullptr, n_chan, max_push_samples, out);
}

extern "C" int bp_lmstream_open_nt(int device, int fea_dim, const bp_logmmse_params *p, const bp_noise_params *np, int n_chan,
                                   int max_push_samples, bp_lmstream **out)
{
    return lmstream_open("bp_lmstream_open_nt", device, fea_dim, p, true, np, n_chan, max_push_samples, out);
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
    { const std::string m = stream_push_checks("bp_lmstream_push", nc, s->max_push, n_in, pcm, &total_in); if (!m.empty()) return fail(BP_ERR_ARG, m); }
    for (int c = 0; c < nc; ++c) {
        ChanStep &p = s->plan[c];
        p = stream_step(hop, 0, init, s->ch[c].received, n_in[c], end && end[c]);
        due += p.c1.so - p.c0.so;
        if (p.c1.fo > p.c0.fo) units += p.c1.fo - p.c0.fo + 1;
    }
    { const std::string m = stream_out_checks("bp_lmstream_push", due, out_cap, out_pcm); if (!m.empty()) return fail(BP_ERR_ARG, m); }
    if ((size_t)units > s->max_units || (size_t)due > s->max_units * hop)
        return fail(BP_ERR_STATE, "bp_lmstream_push: internal: more frames than the stream was sized for");
    // ---- the input block: one job per channel with output frames | their [carry | new] samples at hop-aligned places (the pinned
    // block is reused by every push: the previous one ended in a synchronisation); with it the channels' new carry
    s->jobs.clear();
    char *pin = s->blk.pin_in.as<char>(), *dev = s->blk.dev.as<char>();
    float *hp = (float *)(pin + s->o_pcm);
    size_t unit = 0, src = 0;
    int64_t out_base = 0;
    for (int c = 0; c < nc; ++c) {
        const ChanStep &p = s->plan[c];
        Carry &ch = s->ch[c];
        const float *in = pcm ? pcm + src : nullptr;
        const size_t n = (size_t)n_in[c];
        src += n;
        const int64_t fo0 = p.c0.fo, fo1 = p.c1.fo, nf = fo1 - fo0;
        n_out[c] = (int)(p.c1.so - p.c0.so);
        if (nf > 0) {
            // frame fo0 + i starts at unit + i; zeros behind a sentence's end
            ch.fill_segment(hp + unit * hop, (size_t)(nf + 1) * hop, in, n);
            LmJob j; memset(&j, 0, sizeof(j));
            j.chan = c; j.unit = (int)unit; j.t0 = (int)fo0; j.nf = (int)nf; j.ended = p.ended ? 1 : 0;
            j.out_off = (int)out_base; j.out_n = n_out[c];
            s->jobs.push_back(j);
            unit += (size_t)(nf + 1);
            out_base += n_out[c];
        }
        // the carry: a new sentence starts from hop zeros; else the last hop + r1 - fo1 hop samples of [carry | new]
        if (p.ended) ch.reset(hop);
        else if (n > 0 && !ch.keep_last(in, n, (size_t)hop + (size_t)(p.r1 - fo1 * hop)))
            return fail(BP_ERR_STATE, "bp_lmstream_push: internal: the carry exceeds its capacity");
    }
    if (s->jobs.empty()) return BP_OK;                              // no channel got a new output frame: no device work
    HIPCHK(hipSetDevice(s->device));
    memcpy(pin, s->jobs.data(), s->jobs.size() * sizeof(LmJob));
    char *din = dev + s->o_in;
    HIPCHK(hipMemcpyAsync(din, pin, s->o_pcm + unit * hop * 4, hipMemcpyHostToDevice, s->st));
    LmStreamArgs a; memset(&a, 0, sizeof(a));
    a.jobs = (const LmJob *)din; a.pcm = (const float *)(din + s->o_pcm);
    a.win = (const float *)(dev + s->o_win); a.tw = (const float2 *)(dev + s->o_tw);
    a.lam = (double *)(dev + s->o_lam); a.Ap = (double *)(dev + s->o_Ap); a.pb = s->np.spp ? (double *)(dev + s->o_pb) : nullptr; a.half = (float *)(dev + s->o_half);
    a.out = (float *)(dev + s->o_out);
    a.log2M = s->log2M; a.D = D; a.init_frames = init;
    a.alpha = s->lp.alpha; a.mu = s->lp.mu; a.eta = s->lp.eta; a.xi_min = s->lp.xi_min; a.gamma_max = s->lp.gamma_max; a.np = s->np;
    const dim3 grid((unsigned)s->jobs.size()), blk(WAVE_THREADS);
    const size_t lds = lm_lds_bytes(hop);
    with_nb(D, s->np.spp, [&](auto nb, auto spp) { hipLaunchKernelGGL((bp_lmstream_push<decltype(nb)::value, decltype(spp)::value>), grid, blk, lds, s->st, a); });
    HIPCHK(hipGetLastError());
    HIPCHK(s->blk.copy_back(s->o_out, due, out_pcm, s->st));
    return BP_OK;
}
