// bp_wave.hip -- C-ABI implementation (include/bp_c_api.h), part 4 of 9: the signal layer around the network.  Noisy PCM
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
//   bp_wave_synthesis  per frame: S from the net output and Y, inverse real FFT, times the window -> frames [T][n_fft]
//   bp_wave_overlap    per output sample: the sum over the two covering frames / the sum of squared window values (a gather: no
//                      atomics, the same bits on every run)
#include <hip/hip_runtime.h>
#include <string.h>
#include <cmath>
#include <string>
#include <vector>

#include "bp_fft.h"
#include "bp_handle.h"

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
    if (a.rows && tid == 0) { a.win_start[g] = base + t; if (a.nat_row) a.nat_row[g] = s; }
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

__global__ __launch_bounds__(WAVE_THREADS) void bp_wave_synthesis(const WaveSynArgs a)
{
    extern __shared__ float2 z[];
    const int g = blockIdx.x;
    synth_frame(z, a.out + (size_t)g * a.ldo + a.out_col, a.Y + (size_t)g * a.D, a.win, a.tw, a.log2M, a.target,
                a.frames + ((size_t)g << (a.log2M + 1)));
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

hipError_t wave_synthesis_launch(const float *out, int ldo, int out_col, const float2 *Y, const float *win, const float2 *tw, int log2M,
                                 int D, int target, float *syn, int frames, hipStream_t st)
{
    WaveSynArgs a; memset(&a, 0, sizeof(a));
    a.out = out; a.ldo = ldo; a.out_col = out_col;
    a.Y = Y; a.win = win; a.tw = tw; a.log2M = log2M; a.D = D; a.target = target; a.frames = syn;
    const int M = 1 << log2M;
    hipLaunchKernelGGL(bp_wave_synthesis, dim3((unsigned)frames), dim3(WAVE_THREADS), lds_bytes(M) + (size_t)(M + 1) * sizeof(float2), st, a);
    return hipGetLastError();
}

hipError_t wave_overlap_launch(const float *syn, const float *win, const int *F, int n_sent, int hop, float *pcm, int frames, hipStream_t st)
{
    hipLaunchKernelGGL(bp_wave_overlap, dim3((unsigned)frames), dim3(WAVE_THREADS), 0, st, syn, win, F, n_sent, hop, pcm);
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
    if (c->target != BP_WAVE_LPS && c->target != BP_WAVE_MASK) return fail(BP_ERR_ARG, "bp_enhance_waves: target must be BP_WAVE_LPS or BP_WAVE_MASK");
    if (c->out_col < 0 || (long)c->out_col + D > sL) return fail(BP_ERR_ARG, "bp_enhance_waves: out_col + fea_dim exceeds layersizes[last]");
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
    if ((r = window_reserve(h, rows * D * 4, 0, nat ? (size_t)c->n_sent * D * 4 : 0, p.frames, &rows_d, nullptr, &nat_d, &tab_d)) != BP_OK) return r;
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
        a.Y = Y; a.rows = rows_d; a.win_start = ws_d; a.nat_row = nat ? nr_d : nullptr;
        hipLaunchKernelGGL(bp_wave_analysis, dim3((unsigned)n), dim3(WAVE_THREADS), lds_bytes(p.M), h->stream, a);
        HIPCHK(hipGetLastError());
    }
    if (nat) {
        HIPCHK(wave_nat_launch(rows_d, F, c->n_sent, D, ctx, toff, nat_d, h->stream));
    }
    window_adopt(h, n, D, ctx, nat, false);
    if ((r = forward_resident(h, n)) != BP_OK) return r;
    {
        WaveSynArgs a; memset(&a, 0, sizeof(a));
        a.out = h->out_chunk.as<float>(); a.ldo = h->ld[L - 1]; a.out_col = c->out_col;
        a.Y = Y; a.win = win; a.tw = tw; a.log2M = p.log2M; a.D = D; a.target = c->target; a.frames = (float *)h->wave[2].p;
        hipLaunchKernelGGL(bp_wave_synthesis, dim3((unsigned)n), dim3(WAVE_THREADS), lds_bytes(p.M) + (size_t)(p.M + 1) * sizeof(float2), h->stream, a);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(bp_wave_overlap, dim3((unsigned)n), dim3(WAVE_THREADS), 0, h->stream, (const float *)h->wave[2].p, win, F, c->n_sent, p.hop,
                       (float *)h->wave[3].p);
    HIPCHK(hipGetLastError());
    float *hout = (float *)h->wave_pin[1].p;
    HIPCHK(hipMemcpyAsync(hout, h->wave[3].p, pcm_b, hipMemcpyDeviceToHost, h->stream));
    if (out_net) HIPCHK(hipMemcpyAsync(h->host_out.p, h->out_chunk.p, (size_t)n * h->ld[L - 1] * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    wave_gather(out_pcm, p, c->sent_len, hout);
    if (out_net)
        for (int j = 0; j < n; ++j) memcpy(out_net + (size_t)j * sL, h->host_out.as<float>() + (size_t)j * h->ld[L - 1], sizeof(float) * sL);
    return BP_OK;
}
