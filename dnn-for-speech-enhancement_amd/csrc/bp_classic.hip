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

#include <string>
#include <vector>

#include "bp_classic.h"
#include "bp_fft.h"
#include "bp_handle.h"

namespace {

constexpr double LM_FLOOR = 1e-10;                               // lambda_floor: the LPS floor
constexpr double LM_EULER = 0.57721566490153286061;

struct LogmmseArgs {
    const float2 *Y; const int *F;
    float *gain, *vad;
    int D, init_frames;
    double alpha, mu, eta, xi_min, gamma_max;
};

// E1(x), x > 0: the power series up to x = 1, the continued fraction (modified Lentz) beyond
__device__ double lm_e1(double x)
{
    if (x <= 1.0) {
        double sum = 0.0, term = 1.0;                            // term = (-x)^n / n!
        for (int n = 1; n <= 64; ++n) {
            term *= -x / n;
            const double c = term / n;
            sum += c;
            if (fabs(c) <= 1e-17 * fabs(sum)) break;
        }
        return -LM_EULER - log(x) - sum;
    }
    double b = x + 1.0, c = 1e300, d = 1.0 / b, h = d;
    for (int i = 1; i <= 200; ++i) {
        const double an = -(double)i * i;
        b += 2.0;
        d = 1.0 / (an * d + b);
        c = b + an / c;
        const double del = c * d;
        h *= del;
        if (fabs(del - 1.0) < 1e-16) break;
    }
    return h * exp(-x);
}

__device__ __forceinline__ double lm_power(float2 y) { return (double)y.x * (double)y.x + (double)y.y * (double)y.y; }

__device__ __forceinline__ double lm_wave_sum(double x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

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
    for (int j = 0; j < NB; ++j) lam[j] = fmax(lam[j] / ni, LM_FLOOR);
    float2 cur[NB], nxt[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) cur[j] = Y[kc[j]];
    for (int t = 0; t < T; ++t) {
        const size_t rn = (size_t)(t + 1 < T ? t + 1 : T - 1) * D;
#pragma unroll
        for (int j = 0; j < NB; ++j) nxt[j] = Y[rn + kc[j]];
        double P[NB], gm[NB], xi[NB], part = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            P[j] = lm_power(cur[j]);
            gm[j] = fmin(P[j] / lam[j], a.gamma_max);
            const double dd = t == 0 ? a.alpha : a.alpha * Ap[j] / lam[j];
            xi[j] = fmax(dd + (1.0 - a.alpha) * fmax(gm[j] - 1.0, 0.0), a.xi_min);
            if (on[j]) part += gm[j] * xi[j] / (1.0 + xi[j]) - log(1.0 + xi[j]);
        }
        part = lm_wave_sum(part);
        if ((tid & 63) == 0) red[t & 1][tid >> 6] = part;
        __syncthreads();                                         // (the other set is written next: one barrier per frame)
        const double vad = ((red[t & 1][0] + red[t & 1][1]) + (red[t & 1][2] + red[t & 1][3])) / D;
        const bool noise = vad < a.eta;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (!on[j]) continue;
            const double A = xi[j] / (1.0 + xi[j]), v = A * gm[j];
            const double G = P[j] > 0.0 ? A * exp(0.5 * lm_e1(v)) : 0.0;
            Ap[j] = G * G * P[j];
            gain[(size_t)t * D + tid + j * WAVE_THREADS] = (float)G;
            if (noise) lam[j] = fmax(a.mu * lam[j] + (1.0 - a.mu) * P[j], LM_FLOOR);
        }
        if (tid == 0) a.vad[f0 + t] = (float)vad;
#pragma unroll
        for (int j = 0; j < NB; ++j) cur[j] = nxt[j];
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
