// bp_classic.h -- the log-MMSE recursion of bp_classic.hip, for bp_logmmse_waves and the log-MMSE streams (bp_classic.hip) and
// bp_eval_mix_logmmse (bp_mix.hip).  Definition: include/bp_c_api.h, INTEGRATION.md 1h and 1j.  Internal: nothing in here is part
// of the C ABI.  The MMSE-SPP noise tracker is the second recursion in here: lm_track, run by lm_frame<NB, true>.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "bp_fft.h"
#include "bp_handle.h"

// Checked parameters in the units the kernel uses (xi_min = 10^(xi_min_db / 10)).
struct LogmmseP { double alpha, mu, eta, xi_min, gamma_max; int init_frames; };
// The range rules of bp_logmmse_params (BP_ERR_ARG, nothing touched); p == null: the defaults.
int logmmse_check(const char *who, const bp_logmmse_params *p, LogmmseP &out);
// Checked noise parameters: NoiseP (bp_handle.h: a handle keeps one for bp_set_nat).  spp == false: the VAD-gated update of
// LogmmseP's mu and eta.
// The range rules of bp_noise_params (BP_ERR_ARG, nothing touched); np == null: the defaults of bp_noise_defaults.
int noise_check(const char *who, const bp_noise_params *np, NoiseP &out);
// The NoiseP of the calls without a noise parameter: the VAD-gated update.
inline NoiseP noise_vad() { NoiseP n = {false, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; return n; }
// The recursion over the frames of n_sent sentences (frame prefix F [n_sent + 1], device) of the spectrum Y [frames][D]:
// gain [frames][D] = fl32(G), vad [frames] = fl32(vad_t), noise null or [frames][D] = fl32(the lambda frame t's gamma used).
// One workgroup per sentence.
hipError_t logmmse_gain_launch(const LogmmseP &p, const NoiseP &np, const float2 *Y, const int *F, int n_sent, int D, float *gain, float *vad,
                               float *noise, hipStream_t st);

// ---- the arithmetic of one frame, shared by bp_logmmse_gain (a sentence's frames from a stored spectrum) and bp_lmstream_push
// (a push's frames from PCM to PCM): both return the same bits because both run exactly this.
namespace {

constexpr double LM_FLOOR = 1e-10;                               // lambda_floor: the LPS floor
constexpr double LM_EULER = 0.57721566490153286061;

// E1(x), x > 0: the power series up to x = 1, the continued fraction (modified Lentz) beyond
__device__ __attribute__((unused)) double lm_e1(double x)
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

// (both squares are exact in double: fused or not, one rounding)
__device__ __forceinline__ double lm_power(float2 y) { return (double)y.x * (double)y.x + (double)y.y * (double)y.y; }

__device__ __forceinline__ double lm_wave_sum(double x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// The noise start from the summed power of the sentence's first ni frames
__device__ __forceinline__ double lm_noise_start(double sum, int ni) { return fmax(sum / ni, LM_FLOOR); }

// The tracker's step of one frame (MMSE-SPP, Gerkmann and Hendriks 2012, with the ramped ceiling of INTEGRATION.md 1n), in front of
// the frame's gain: lam and pb (the smoothed presence probability, 0 at a sentence's start) of the thread's bins, updated in place.
// No decision in here: min, max and the clamp only.  A bin that does not exist repeats bin D - 1 (its y is that bin's).
template <int NB>
__device__ __forceinline__ void lm_track(const NoiseP &n, const float2 (&y)[NB], double (&lam)[NB], double (&pb)[NB])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const double P = lm_power(y[j]);
        double ph = 1.0 / (1.0 + n.c0 * exp(-n.c1 * P / lam[j]));
        pb[j] = n.a_spp * pb[j] + (1.0 - n.a_spp) * ph;
        const double r = fmin(fmax((pb[j] - n.p_lo) / (n.p_cap - n.p_lo), 0.0), 1.0);
        ph = fmin(ph, 1.0 - (1.0 - n.p_cap) * r);
        lam[j] = fmax(n.a_pow * lam[j] + (1.0 - n.a_pow) * ((1.0 - ph) * P + ph * lam[j]), LM_FLOOR);
    }
}

// One frame of the dynamic noise-aware input of one bin: the tracker's step on y, then the normalised LPS of
// fl32(lambda) in the expression of the noisy row.  bp_wave_dnat (bp_wave.hip) and bp_stream_dnat (bp_stream.hip) run exactly this per frame.
__device__ __forceinline__ float lm_dnat(const NoiseP &n, float2 y, double &lam, double &pb, float mean, float inv_std)
{
#pragma clang fp contract(off)
    const float2 yy[1] = {y};
    double l[1] = {lam}, p[1] = {pb};
    lm_track<1>(n, yy, l, p);
    lam = l[0]; pb = p[0];
    return (lps_of((float)lam) - mean) * inv_std;
}

// One frame of the recursion for a workgroup of WAVE_THREADS threads, thread i owning bins i, i + WAVE_THREADS, ... (on[j]: the
// bin exists; y[j] of a bin that does not is any finite value).  first: frame 0 of its sentence.  lam / Ap: the thread's noise
// estimate and A_prev, updated in place; red: WAVE_THREADS / 64 LDS slots that no thread touches again before the workgroup's
// next barrier but one (callers alternate two sets, or have barriers of their own between frames).  Contains one barrier.
// Returns vad_t; g[j] = fl32(G) of the bins that exist, nz[j] = fl32(the lambda the frame's gamma used).
// SPP: lm_track (n, pb) moves lambda in front of the gain and the VAD-gated update behind it is gone (mu and eta take no part);
// the instantiation without it reads neither n nor pb.
// The contraction is spelled out -- fma() where bp_logmmse_gain fused before this function existed, nothing else fuses -- because
// which of two products the compiler folds into a sum depends on the code around a call (bp_fft.h, overlap4).
template <int NB, bool SPP>
__device__ __forceinline__ double lm_frame(double alpha, double mu, double eta, double xi_min, double gamma_max, const NoiseP &n, int D,
                                           bool first, const float2 (&y)[NB], const bool (&on)[NB], double (&lam)[NB], double (&Ap)[NB],
                                           double (&pb)[NB], double *red, float (&g)[NB], float (&nz)[NB])
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    double P[NB], gm[NB], xi[NB], part = 0.0;
    if (SPP) lm_track<NB>(n, y, lam, pb);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        nz[j] = (float)lam[j];
        P[j] = lm_power(y[j]);
        gm[j] = fmin(P[j] / lam[j], gamma_max);
        const double dd = first ? alpha : alpha * Ap[j] / lam[j];
        xi[j] = fmax(fma(1.0 - alpha, fmax(gm[j] - 1.0, 0.0), dd), xi_min);
        if (on[j]) part += gm[j] * xi[j] / (1.0 + xi[j]) - log(1.0 + xi[j]);
    }
    part = lm_wave_sum(part);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    const double vad = ((red[0] + red[1]) + (red[2] + red[3])) / D;
    const bool noise = vad < eta;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (!on[j]) continue;
        const double A = xi[j] / (1.0 + xi[j]), v = A * gm[j];
        const double G = P[j] > 0.0 ? A * exp(0.5 * lm_e1(v)) : 0.0;
        Ap[j] = G * G * P[j];
        g[j] = (float)G;
        if (!SPP && noise) lam[j] = fmax(fma(1.0 - mu, P[j], mu * lam[j]), LM_FLOOR);
    }
    return vad;
}

}  // namespace
