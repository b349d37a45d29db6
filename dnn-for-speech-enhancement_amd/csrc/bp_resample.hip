// bp_resample.hip -- C-ABI implementation (include/bp_c_api.h): rational sample-rate conversion, so corpora and files of any rate
// work (bp_resample_waves and the bp_resample_* host functions).  No handle: the call runs in a OneShot of
// bp_handle.h.  The kernel's arguments, the plan of a call and the launcher are declared in bp_resample.h.  gfx950 only.
//
// Kernel:
//   bp_wave_resample   per output sample one lane's serial sum in double over its polyphase taps, the workgroup's input span staged
//                      in LDS where it fits
#include <hip/hip_runtime.h>
#include <string.h>
#include <cmath>
#include <string>
#include <vector>

#include "bp_fft.h"
#include "bp_handle.h"
#include "bp_resample.h"

// One lane per output sample k of sentence s: t0 = k q + Lh, phase r = t0 mod p, and the terms h[r + i p] x[t0 / p - i] for
// i ascending -- the order of the definition -- while the tap exists and the sample lies in [0, n).  The products are exact in
// double, so fma and multiply-then-add give the same bits.  The workgroup's samples [i_lo, i_hi] come from LDS (a.lds: staged with
// 16-byte loads from the quad below i_lo on; the host has checked that every workgroup's span fits) or straight from global.
__global__ __launch_bounds__(RS_BLOCK) void bp_wave_resample(const ResampleArgs a)
{
    extern __shared__ __align__(16) float rs_x[];
    const int s = sentence_of(a.rb, a.n_sent, blockIdx.x), tid = threadIdx.x;
    const int n = a.len[s], n_out = a.oo[s + 1] - a.oo[s];
    const int k0 = (blockIdx.x - a.rb[s]) * RS_BLOCK, k = k0 + tid;
    const float *x = a.pcm + a.off[s];
    int64_t base = 0;
    if (a.lds) {
        const int k1 = (k0 + RS_BLOCK < n_out ? k0 + RS_BLOCK : n_out) - 1;             // the workgroup's last output sample
        const int64_t t_lo = (int64_t)k0 * a.q - a.Lh, t_hi = (int64_t)k1 * a.q + a.Lh;  // k0 q + Lh - 2 Lh .. k1 q + Lh
        const int64_t i_lo = t_lo <= 0 ? 0 : (t_lo + a.p - 1) / a.p, i_top = t_hi / a.p, i_hi = i_top < n ? i_top : n - 1;
        base = i_lo & ~(int64_t)3;
        const int quads = i_hi >= base ? (int)((i_hi - base) / 4) + 1 : 0;              // (the padding behind the sentence is zeros)
        for (int c = tid; c < quads; c += RS_BLOCK)
            *reinterpret_cast<float4 *>(rs_x + 4 * c) = *reinterpret_cast<const float4 *>(x + base + 4 * c);
        __syncthreads();
    }
    if (k >= n_out) return;
    const int64_t t0 = (int64_t)k * a.q + a.Lh;
    const int r = (int)(t0 % a.p);
    int64_t i = t0 / a.p;
    int m = 0;
    if (i >= n) { m = (int)(i - n + 1); i = n - 1; }                                    // the taps that meet samples behind the end
    const int cnt = (a.taps - 1 - r) / a.p + 1;                                         // taps of phase r
    const int64_t last = (int64_t)m + i + 1;                                            // ... and those that meet samples before 0
    const int m_end = last < cnt ? (int)last : cnt;
    const float *h = a.hp + (size_t)r * a.tpp;
    double acc = 0.0;
    if (a.lds) {
        const float *xw = rs_x + (i - base);
#pragma unroll 4
        for (; m < m_end; ++m, --xw) acc = fma((double)h[m], (double)*xw, acc);
    } else {
        const float *xw = x + i;
#pragma unroll 4
        for (; m < m_end; ++m, --xw) acc = fma((double)h[m], (double)*xw, acc);
    }
    a.out[(size_t)a.oo[s] + k] = (float)acc;
}

// ------------------------------------------------------------------ host side
namespace {

const int RS_MAX_RATIO = 1024;

// I0(x) = sum_k ((x/2)^k / k!)^2, summed until a term no longer changes the sum
double rs_bessel_i0(double x)
{
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 1000; ++k) {
        t *= (x / (2.0 * k)) * (x / (2.0 * k));
        const double s1 = s + t;
        if (s1 == s) break;
        s = s1;
    }
    return s;
}

int rs_check_params(const char *who, const bp_resample_params *in, bp_resample_params &prm)
{
    if (in) prm = *in; else bp_resample_defaults(&prm);
    if (prm.zeros < 1 || prm.zeros > 32) return fail(BP_ERR_ARG, std::string(who) + ": zeros outside [1, 32]");
    if (!(prm.beta >= 0.0 && prm.beta <= 20.0)) return fail(BP_ERR_ARG, std::string(who) + ": beta outside [0, 20]");
    if (!(prm.rolloff > 0.0 && prm.rolloff <= 1.0)) return fail(BP_ERR_ARG, std::string(who) + ": rolloff outside (0, 1]");
    return BP_OK;
}

// h[0 .. 2 zeros max(p, q)] of checked arguments
void rs_taps(int p, int q, const bp_resample_params &prm, float *h)
{
    const int mx = p > q ? p : q, Lh = prm.zeros * mx, taps = 2 * Lh + 1;
    const double pi = 3.141592653589793238462643383279502884, i0b = rs_bessel_i0(prm.beta);
    std::vector<double> g((size_t)taps);
    double sum = 0.0;
    for (int j = 0; j < taps; ++j) {
        const double u = (double)(j - Lh) / (double)Lh, kw = rs_bessel_i0(prm.beta * sqrt(fmax(0.0, 1.0 - u * u))) / i0b;
        const double v = prm.rolloff * (double)(j - Lh) / (double)mx, sc = v == 0.0 ? 1.0 : sin(pi * v) / (pi * v);
        g[j] = kw * sc; sum += g[j];
    }
    for (int j = 0; j < taps; ++j) h[j] = (float)((double)p * g[j] / sum);
}

}  // namespace

extern "C" int bp_resample_defaults(bp_resample_params *p)
{
    if (!p) return fail(BP_ERR_ARG, "bp_resample_defaults: null pointer");
    p->zeros = 16; p->beta = 8.6; p->rolloff = 0.9;
    return BP_OK;
}

extern "C" int bp_resample_ratio(int rate_in, int rate_out, int *p, int *q)
{
    if (!p || !q) return fail(BP_ERR_ARG, "bp_resample_ratio: null pointer");
    if (rate_in < 1 || rate_out < 1) return fail(BP_ERR_ARG, "bp_resample_ratio: sample rates must be >= 1");
    int a = rate_in, b = rate_out;
    while (b) { const int t = a % b; a = b; b = t; }
    const int pp = rate_out / a, qq = rate_in / a;
    if (pp > RS_MAX_RATIO || qq > RS_MAX_RATIO)
        return fail(BP_ERR_ARG, "bp_resample_ratio: " + std::to_string(rate_in) + " Hz -> " + std::to_string(rate_out) + " Hz is " + std::to_string(pp) +
                                    "/" + std::to_string(qq) + " in lowest terms, and neither may exceed " + std::to_string(RS_MAX_RATIO));
    *p = pp; *q = qq;
    return BP_OK;
}

extern "C" int bp_resample_len(int64_t n, int p, int q, int64_t *n_out)
{
    if (!n_out) return fail(BP_ERR_ARG, "bp_resample_len: null pointer");
    if (p < 1 || p > RS_MAX_RATIO || q < 1 || q > RS_MAX_RATIO) return fail(BP_ERR_ARG, "bp_resample_len: p and q must lie in [1, 1024]");
    if (n < 1 || n > INT64_MAX / (2 * RS_MAX_RATIO)) return fail(BP_ERR_ARG, "bp_resample_len: n outside [1, 2^52]");
    *n_out = (n * p + q - 1) / q;
    return BP_OK;
}

extern "C" int bp_resample_taps(int p, int q, const bp_resample_params *params, float *h, int n_taps)
{
    if (p < 1 || p > RS_MAX_RATIO || q < 1 || q > RS_MAX_RATIO) return fail(BP_ERR_ARG, "bp_resample_taps: p and q must lie in [1, 1024]");
    bp_resample_params prm;
    { const int r = rs_check_params("bp_resample_taps", params, prm); if (r != BP_OK) return r; }
    if (!h) return fail(BP_ERR_ARG, "bp_resample_taps: null output");
    const int want = 2 * prm.zeros * (p > q ? p : q) + 1;
    if (n_taps != want) return fail(BP_ERR_ARG, "bp_resample_taps: n_taps must be 2*zeros*max(p,q)+1 = " + std::to_string(want));
    rs_taps(p, q, prm, h);
    return BP_OK;
}

void resample_plan(int p, int q, const bp_resample_params &prm, int n_sent, const int *sent_len, ResamplePlan &rp)
{
    const int mx = p > q ? p : q;
    rp.p = p; rp.q = q; rp.Lh = prm.zeros * mx; rp.taps = 2 * rp.Lh + 1; rp.tpp = (rp.taps + p - 1) / p;
    std::vector<float> h((size_t)rp.taps);
    rs_taps(p, q, prm, h.data());
    rp.hp.assign((size_t)p * rp.tpp, 0.0f);
    for (int j = 0; j < rp.taps; ++j) rp.hp[(size_t)(j % p) * rp.tpp + j / p] = h[j];
    rp.off.assign((size_t)n_sent, 0); rp.oo.assign((size_t)n_sent + 1, 0); rp.rb.assign((size_t)n_sent + 1, 0);
    int64_t at = 0;
    for (int s = 0; s < n_sent; ++s) {
        const int64_t no = ((int64_t)sent_len[s] * p + q - 1) / q;
        rp.off[s] = at; at += ((int64_t)sent_len[s] + 3) & ~(int64_t)3;
        rp.oo[s + 1] = rp.oo[s] + (int)no;
        rp.rb[s + 1] = rp.rb[s] + (int)((no + RS_BLOCK - 1) / RS_BLOCK);
    }
    rp.in_floats = (size_t)at;
    // a workgroup reads at most ((RS_BLOCK - 1) q + 2 Lh) / p + 1 samples, from the quad below the first to the quad's end behind the last
    const int64_t need = ((int64_t)(RS_BLOCK - 1) * q + 2 * (int64_t)rp.Lh) / p + 8;
    rp.lds = need <= RS_LDS_FLOATS;
    rp.lds_bytes = rp.lds ? (size_t)((need + 3) & ~(int64_t)3) * 4 : 0;
}

hipError_t resample_launch(const ResampleArgs &a, const ResamplePlan &rp, hipStream_t st)
{
    hipLaunchKernelGGL(bp_wave_resample, dim3((unsigned)rp.rb.back()), dim3(RS_BLOCK), rp.lds_bytes, st, a);
    return hipGetLastError();
}

extern "C" int bp_resample_waves(int device, int rate_in, int rate_out, const bp_resample_params *params, int n_sent, const int *sent_len,
                                 const float *pcm, float *out)
{
    int p = 0, q = 0;
    if (bp_resample_ratio(rate_in, rate_out, &p, &q) != BP_OK) return fail(BP_ERR_ARG, "bp_resample_waves: " + g_bp_err);
    bp_resample_params prm;
    { const int r = rs_check_params("bp_resample_waves", params, prm); if (r != BP_OK) return r; }
    if (n_sent < 1 || !sent_len || !pcm || !out) return fail(BP_ERR_ARG, "bp_resample_waves: no sentences or null pointer");
    int64_t tot_in = 0, tot_out = 0;
    for (int s = 0; s < n_sent; ++s) {
        if (sent_len[s] < 1) return fail(BP_ERR_ARG, "bp_resample_waves: empty sentence " + std::to_string(s));
        tot_in += sent_len[s]; tot_out += ((int64_t)sent_len[s] * p + q - 1) / q;
        if (tot_out > INT32_MAX) return fail(BP_ERR_ARG, "bp_resample_waves: 2^31 output samples or more in one call");
    }
    if (p == q) { memmove(out, pcm, (size_t)tot_in * 4); return BP_OK; }     // the input's bits; nothing is filtered
    ResamplePlan rp;
    resample_plan(p, q, prm, n_sent, sent_len, rp);
    Layout lay;                                                              // off | len | oo | rb | taps | pcm, then the output
    const size_t o_off = lay.take(rp.off.size() * 8), o_len = lay.take((size_t)n_sent * 4), o_oo = lay.take(rp.oo.size() * 4);
    const size_t o_rb = lay.take(rp.rb.size() * 4), o_hp = lay.take(rp.hp.size() * 4), o_pcm = lay.take(rp.in_floats * 4);
    const size_t in_b = lay.size(), out_b = (size_t)tot_out * 4;
    OneShot os;
    { const int r = os.open("bp_resample_waves", device, in_b + out_b); if (r != BP_OK) return r; }
    std::vector<char> hb(in_b, 0);
    memcpy(hb.data() + o_off, rp.off.data(), rp.off.size() * 8);
    memcpy(hb.data() + o_len, sent_len, (size_t)n_sent * 4);
    memcpy(hb.data() + o_oo, rp.oo.data(), rp.oo.size() * 4);
    memcpy(hb.data() + o_rb, rp.rb.data(), rp.rb.size() * 4);
    memcpy(hb.data() + o_hp, rp.hp.data(), rp.hp.size() * 4);
    { const float *src = pcm; for (int s = 0; s < n_sent; src += sent_len[s++]) memcpy(hb.data() + o_pcm + (size_t)rp.off[s] * 4, src, (size_t)sent_len[s] * 4); }
    hipError_t &e = os.e;
    char *d = os.d.as<char>();
    if (e == hipSuccess) e = hipMemcpyAsync(d, hb.data(), in_b, hipMemcpyHostToDevice, os.st);
    if (e == hipSuccess) {
        ResampleArgs a; memset(&a, 0, sizeof(a));
        a.pcm = (const float *)(d + o_pcm); a.hp = (const float *)(d + o_hp); a.off = (const int64_t *)(d + o_off);
        a.len = (const int *)(d + o_len); a.oo = (const int *)(d + o_oo); a.rb = (const int *)(d + o_rb); a.out = (float *)(d + in_b);
        a.n_sent = n_sent; a.p = p; a.q = q; a.Lh = rp.Lh; a.taps = rp.taps; a.tpp = rp.tpp; a.lds = rp.lds;
        e = resample_launch(a, rp, os.st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + in_b, out_b, hipMemcpyDeviceToHost, os.st);
    return os.finish("bp_resample_waves");
}
