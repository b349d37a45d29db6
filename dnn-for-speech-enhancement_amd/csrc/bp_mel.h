// bp_mel.h -- the MFCC auxiliary target (include/bp_c_api.h): the checked parameters, the two host tables
// (mel filters and the liftered DCT, computed in double and rounded to fp32 once), the block the device reads them from, and the
// launcher of bp_wave_mel (bp_wave.hip) -- the one kernel behind bp_wave_mfcc and the MFCC columns of the mixing calls
// (bp_set_mix_aux, bp_mix.hip).  Internal: nothing in here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "bp_fft.h"
#include "bp_handle.h"

// (MelP, the checked parameters, and MEL_MAX: bp_handle.h -- the handle keeps a copy)

// The tables of one (fea_dim, MelP): w dense [n_mel][D] as bp_mel_filters returns it, the bins with w > 0 of every filter, t [n_ceps][n_mel]
struct MelTab {
    int D, n_mel, n_ceps;
    std::vector<float> w, t;
    std::vector<int> first, nb;
};

// What the kernel reads, one device block: off | first | nb [n_mel] (filter j's weights are wp[off[j] .. off[j] + nb[j]), for the
// bins first[j] ...), wp the weights of all filters back to back, tT the DCT table transposed [n_mel][n_ceps] (thread r reads
// tT[j n_ceps + r]: neighbours for neighbouring r), mean | scale [n_ceps]
struct MelDev { const int *off, *first, *nb; const float *wp, *tT, *mean, *scale; int n_mel, n_ceps; };
struct MelBlock { size_t off, first, nb, wp, tT, mean, scale, bytes; };

// bp_wave_mel arguments: frame g of sentence s reads the padded samples [(g + s) hop, (g + s) hop + n_fft), as bp_wave_analysis does
struct MelArgs {
    const float *pcm; const float *win; const float2 *tw; const int *F;
    int n_sent, log2M, D, hop;
    MelDev m;
    float *power, *logmel;        // [frames][D], [frames][n_mel], or null
    float *mfcc; int ldm, col;    // row g's coefficients at mfcc[g ldm + col ...), or null
};
hipError_t wave_mel_launch(const MelArgs &a, int frames, hipStream_t st);

inline int mel_check(const char *who, const bp_mel_params *p, MelP &m)
{
    const std::string w(who);
    if (!p) return fail(BP_ERR_ARG, w + ": null parameters");
    if (p->sample_rate < 1) return fail(BP_ERR_ARG, w + ": sample_rate must be > 0");
    if (p->n_mel < 2 || p->n_mel > MEL_MAX) return fail(BP_ERR_ARG, w + ": n_mel outside [2, 128]");
    if (p->first_coef != 0 && p->first_coef != 1) return fail(BP_ERR_ARG, w + ": first_coef must be 0 or 1");
    if (p->n_ceps < 1 || p->n_ceps > p->n_mel - p->first_coef) return fail(BP_ERR_ARG, w + ": n_ceps outside [1, n_mel - first_coef]");
    if (!(p->f_lo >= 0.0f && p->f_lo < p->f_hi && (double)p->f_hi <= 0.5 * (double)p->sample_rate))
        return fail(BP_ERR_ARG, w + ": need 0 <= f_lo < f_hi <= sample_rate / 2");
    if (!(p->lifter >= 0.0f) || !std::isfinite(p->lifter)) return fail(BP_ERR_ARG, w + ": lifter must be finite and >= 0");
    memset(&m, 0, sizeof(m));
    m.sample_rate = p->sample_rate; m.n_mel = p->n_mel; m.n_ceps = p->n_ceps; m.first_coef = p->first_coef;
    m.f_lo = p->f_lo; m.f_hi = p->f_hi; m.lifter = p->lifter;
    for (int r = 0; r < p->n_ceps; ++r) {
        m.mean[r] = p->mean ? p->mean[r] : 0.0f; m.scale[r] = p->scale ? p->scale[r] : 1.0f;
        if (!std::isfinite(m.mean[r]) || !std::isfinite(m.scale[r])) return fail(BP_ERR_ARG, w + ": mean / scale entry " + std::to_string(r) + " is not finite");
    }
    return BP_OK;
}

inline double mel_of_hz(double f) { return 2595.0 * log10(1.0 + f / 700.0); }
inline double hz_of_mel(double m) { return 700.0 * (pow(10.0, m / 2595.0) - 1.0); }

// t[r][j] = lift_i sqrt(2 / n_mel) cos(pi i (j + 0.5) / n_mel), i = first_coef + r
inline void mel_dct(const MelP &m, float *t)
{
    const double pi = 3.141592653589793238462643383279502884;
    for (int r = 0; r < m.n_ceps; ++r) {
        const int i = m.first_coef + r;
        const double lift = m.lifter > 0.0 ? 1.0 + 0.5 * m.lifter * sin(pi * (double)i / m.lifter) : 1.0;
        for (int j = 0; j < m.n_mel; ++j)
            t[(size_t)r * m.n_mel + j] = (float)(lift * sqrt(2.0 / (double)m.n_mel) * cos(pi * (double)i * ((double)j + 0.5) / (double)m.n_mel));
    }
}

// The tables of checked parameters at fea_dim (a valid one).  Edges: e_0 = f_lo and e_{n_mel+1} = f_hi as given, those between them
// equally spaced in mel and mapped back to Hz.  BP_ERR_ARG, naming the filter, when a filter has no bin with w > 0.
inline int mel_tables(const char *who, int fea_dim, const MelP &m, MelTab &tab)
{
    const int D = fea_dim, n = m.n_mel;
    tab.D = D; tab.n_mel = n; tab.n_ceps = m.n_ceps;
    tab.w.assign((size_t)n * D, 0.0f); tab.first.assign((size_t)n, 0); tab.nb.assign((size_t)n, 0);
    std::vector<double> e((size_t)n + 2);
    const double mlo = mel_of_hz(m.f_lo), mhi = mel_of_hz(m.f_hi);
    for (int p = 0; p <= n + 1; ++p) e[p] = hz_of_mel(mlo + (mhi - mlo) * (double)p / (double)(n + 1));
    e[0] = m.f_lo; e[n + 1] = m.f_hi;
    for (int j = 0; j < n; ++j) {
        int first = -1, last = -1;
        for (int k = 0; k < D; ++k) {
            const double f = (double)k * (double)m.sample_rate / (double)(2 * (D - 1));
            const double up = (f - e[j]) / (e[j + 1] - e[j]), down = (e[j + 2] - f) / (e[j + 2] - e[j + 1]);
            const float w = (float)fmax(0.0, fmin(up, down));
            tab.w[(size_t)j * D + k] = w;
            if (w > 0.0f) { if (first < 0) first = k; last = k; }
        }
        if (first < 0)
            return fail(BP_ERR_ARG, std::string(who) + ": mel filter " + std::to_string(j) + " holds no bin (fea_dim " + std::to_string(D) + ", " +
                                        std::to_string(m.sample_rate) + " Hz, " + std::to_string(n) + " filters): fewer filters or a larger fea_dim");
        tab.first[j] = first; tab.nb[j] = last - first + 1;
    }
    tab.t.resize((size_t)m.n_ceps * n);
    mel_dct(m, tab.t.data());
    return BP_OK;
}

// the device block of (n_mel, n_ceps) with n_w packed weights; every block fits the one of mel_block(MEL_MAX, MEL_MAX, 2 * 1025): a
// bin lies under at most two triangles
inline MelBlock mel_block(int n_mel, int n_ceps, size_t n_w)
{
    MelBlock b;
    Layout lay;
    b.off = lay.take((size_t)n_mel * 4); b.first = lay.take((size_t)n_mel * 4); b.nb = lay.take((size_t)n_mel * 4);
    b.wp = lay.take(n_w * 4); b.tT = lay.take((size_t)n_mel * n_ceps * 4);
    b.mean = lay.take((size_t)n_ceps * 4); b.scale = lay.take((size_t)n_ceps * 4);
    b.bytes = lay.size();
    return b;
}
inline size_t mel_block_limit() { return mel_block(MEL_MAX, MEL_MAX, (size_t)2 * 1025).bytes; }

inline size_t mel_packed_weights(const MelTab &tab)
{
    size_t n = 0;
    for (int j = 0; j < tab.n_mel; ++j) n += (size_t)tab.nb[j];
    return n;
}

// fills hb (b.bytes, from mel_block(n_mel, n_ceps, mel_packed_weights(tab))); the pointers of MelDev are then dev + the offsets
inline void mel_block_fill(char *hb, const MelBlock &b, const MelP &m, const MelTab &tab)
{
    int *off = (int *)(hb + b.off);
    float *wp = (float *)(hb + b.wp), *tT = (float *)(hb + b.tT);
    int at = 0;
    for (int j = 0; j < tab.n_mel; ++j) {
        off[j] = at;
        memcpy(wp + at, tab.w.data() + (size_t)j * tab.D + tab.first[j], (size_t)tab.nb[j] * 4);
        at += tab.nb[j];
    }
    memcpy(hb + b.first, tab.first.data(), (size_t)tab.n_mel * 4);
    memcpy(hb + b.nb, tab.nb.data(), (size_t)tab.n_mel * 4);
    for (int r = 0; r < tab.n_ceps; ++r)
        for (int j = 0; j < tab.n_mel; ++j) tT[(size_t)j * tab.n_ceps + r] = tab.t[(size_t)r * tab.n_mel + j];
    memcpy(hb + b.mean, m.mean, (size_t)tab.n_ceps * 4);
    memcpy(hb + b.scale, m.scale, (size_t)tab.n_ceps * 4);
}

inline MelDev mel_dev(const char *dev, const MelBlock &b, const MelTab &tab)
{
    MelDev d;
    d.off = (const int *)(dev + b.off); d.first = (const int *)(dev + b.first); d.nb = (const int *)(dev + b.nb);
    d.wp = (const float *)(dev + b.wp); d.tT = (const float *)(dev + b.tT);
    d.mean = (const float *)(dev + b.mean); d.scale = (const float *)(dev + b.scale);
    d.n_mel = tab.n_mel; d.n_ceps = tab.n_ceps;
    return d;
}
