// bp_eval.hip -- C-ABI implementation (include/bp_c_api.h): objective scores of enhanced speech, estimates against a reference, in
// score rows of one of the widths of EVAL_WIDTHS (bp_eval.h: which columns and kernels each width adds; bp_score_waves[_ext] here,
// bp_eval_mix[_ext] in bp_mix.hip through bp_eval.h).  Definitions: include/bp_c_api.h, INTEGRATION.md 1f.  gfx950 only.
// bp_score_waves takes its frame plan and padded layout from bp_wave.hip (plan_waves, wave_scatter: bp_fft.h) and its stream and
// device block from OneShot (bp_handle.h).  Host side: the prefix tables are named once in EVAL_PRE (bp_eval.h), the work arrays
// once in work_rows, and the table and work blocks are laid out and bound to the kernels' argument block by walking those.
//
// Kernels (signal 0 is the reference, 1 .. nsig-1 the estimates; blockIdx.y picks the signal; a flat grid of workgroups finds its
// sentence by a binary search over a prefix table, as bp_wave_analysis does over F):
//   bp_eval_resample  per 10 kHz output sample: the polyphase sum of scipy's resample_poly (taps in double on the host), in double
//   bp_eval_energy    reference only, one wave64 per STOI frame: E_j = sum (v r)^2 in double (a fixed shuffle tree)
//   bp_eval_mask      reference only, one workgroup per sentence: max E, the 40 dB rule, the ranks of the kept frames (LDS scan)
//   bp_eval_compact   per compacted sample: the (at most two) kept frames that overlap it, the earlier one added first
//   bp_eval_bands     one workgroup per STFT frame: rfft_frame / rfft_bin of bp_fft.h at 512 points, 15 band envelopes
//   bp_eval_corr      per (segment, band) pair of an estimate: the clipped, normalised correlation over 30 frames, in double
//   bp_eval_ssnr      one wave64 per SSNR frame of an estimate: E_s, E_d in double, the clamped frame SNR
//   bp_eval_lsd       one wave64 per analysis frame of an estimate: the RMS of the dB difference of the two LPS rows, in double
//   bp_eval_estoi     five columns only, one wave64 per segment: the 15 x 30 envelope matrices of every signal in LDS, rows then
//                     columns normalised in double (the reference's once), d_m of every estimate (a fixed shuffle tree)
//   bp_eval_sisdr     five columns only, one workgroup per (sentence, estimate): rr, er, then with alpha num, den -- two passes
//                     over the samples in double (strided sums, a fixed LDS tree)
//   bp_eval_reduce    one workgroup per (sentence, estimate): the means in double (strided sums, a fixed LDS tree), one score row
//   bp_eval_lpc<P>    seven columns only, one workgroup per 32 SSNR frames of the call: per (signal, frame) one wave64 puts the
//                     windowed frame into LDS in double and sums the P + 1 autocorrelation lags (4 lag groups x 16 sample segments
//                     over the lanes, a fixed shuffle tree over the segments); then one thread per (signal, frame) runs the Levinson-Durbin recursion and the LPC
//                     cepstrum in registers (the reference's once, shared through LDS) and the quadratic forms: LLR_j, CD_j, valid_j
//   bp_eval_lpcrank   seven columns and up, rank-and-select, one thread per SSNR frame of an estimate: the frame's rank among the
//                     sentence's valid frames in each of the one or two measures that a.rank names for the launch (integer counts;
//                     the sentence's values pass through LDS in tiles), selected iff rank < Jk
//   bp_eval_lpcsum    seven columns only, one workgroup per (sentence, estimate): the selected values summed (strided sums, a
//                     fixed LDS tree), divided by Jk: columns 5 and 6
//   bp_eval_cb        nine columns only, one workgroup per 16 SSNR frames of the call: per (signal, frame), 1 to 4 of them at a time
//                     (64 to 256 threads each, by n_fft), the windowed frame, zero-padded to n_fft, as a complex FFT of n_fft / 2
//                     points in LDS in double (twiddles from a host double table) and the split step, |X| and |X|^2 in place; sum |X|
//                     (strided sums, a fixed shuffle tree) and the 25 sparse band sums of both kinds (2 to 8 lanes per band, a fixed
//                     shuffle tree) into LDS as [signal][band][frame], the reference's once; then 32 lanes per (estimate, frame), one per
//                     band, do the 25-band part (a fixed shuffle tree over the bands): fwSegSNR_j, WSS_j and their validity
//   bp_eval_cbsum     nine columns only, one workgroup per (sentence, estimate): the valid fwSegSNR values and the WSS values that
//                     bp_eval_lpcrank selected (a second launch, ranking the WSS values alone) summed (strided sums, a fixed LDS
//                     tree): columns 7 and 8
//   bp_eval_trim      per padded sample: zero outside the sentence (the overlap-add output, before it is analysed)
// No float atomics and no cross-workgroup hand-off inside a kernel: the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "bp_eval.h"
#include "bp_fft.h"
#include "bp_handle.h"

namespace {

constexpr int EV_N = 256, EV_K = 128, EV_NFFT = 512, EV_NB = 15, EV_BS = 16, EV_SEG = 30;   // STOI frame, hop, FFT, bands, band stride, segment
constexpr int EV_LOG2M = 8;                                                                 // rfft_frame: 512 points as 256 complex
constexpr double EV_EPS = 2.220446049250313e-16;
__constant__ int ev_band_lo[EV_NB] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
__constant__ int ev_band_hi[EV_NB] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
constexpr int EV_BIN_LO = 7, EV_BIN_HI = 219;

// What one bp_eval_lpcrank launch ranks: nval (1 or 2) arrays of per-frame values [est][SJ[n]], their frames' validity, and where
// the selection goes (bit k: selected in val[k])
struct RankSel { const double *val[2]; int nval; const int *valid; int *sel; };

struct EvalArgs {
    const int64_t *off; const int *len;
#define X(name) const int *name;
    EVAL_PRE(X)                                              // a.o10 .. a.FS
#undef X
    const float *h, *v; const float2 *tw; const double *w;
    int n, p, q, Lh, taps, win, skip, D;
    double clip;                                             // 1 + 10^(15/20)
    const float *sig[EVAL_MAXSIG], *lps[EVAL_MAXSIG];
    float *r10; size_t s10;                                  // [sig][o10[n]]
    double *E; int *frm, *C;                                 // [P[n]], [P[n]], [n]
    float *comp; size_t scomp;                               // [sig][Q[n]]
    float *band; size_t sband;                               // [sig][P[n]][EV_BS]
    double *rho, *ssnr, *lsd; size_t srho, sssnr, slsd;      // [est][CP[n]], [est][SJ[n]], [est][F[n]]
    double *dm, *sdr; size_t sdm; int nsig;                  // five columns: [est][CP[n] / 15], [est][n]
    double *llr, *lcd; int *lv, *lsel;                       // seven columns: [est][SJ[n]] each (lv: valid; lsel: bit 0 LLR, bit 1 CD selected)
    // nine columns: twiddles exp(-2 pi i j / n_fft) [cH + 1]; per band first bin, bins, offset into cg [3][25]; the weights; n_fft / 2
    const double2 *ctw; const int *cband; const double *cg; int cH;
    double *fw, *ws; int *fv, *wv, *csel;                    // [est][SJ[n]] each (fv, wv: valid; csel: bit 0 WSS selected)
    float *scores; int ns;                                   // [est][n][ns]
    RankSel rank;                                            // set per bp_eval_lpcrank launch
};

__device__ __forceinline__ double wave_sum(double x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

struct OpAdd { __device__ double operator()(double x, double y) const { return x + y; } };
struct OpMax { __device__ double operator()(double x, double y) const { return fmax(x, y); } };
constexpr float EV_NAN = __builtin_bit_cast(float, 0x7fc00000);   // the score of an undefined measure

// The block reduction of the per-sentence kernels: ND doubles (combined by op) and NI ints (added) over the WAVE_THREADS threads by
// the fixed LDS tree -- strides 128, 64, .. 1, thread tid < w takes in thread tid + w.  q and c: the thread's own results on entry
// (its strided partial sums, formed in ascending order), the block's on return, in every thread.  A kernel that reduces twice puts
// a barrier between the two: the LDS is the same.
template <int ND, int NI, class Op = OpAdd> __device__ __forceinline__ void block_reduce(double *q, int *c, Op op = Op())
{
    __shared__ __align__(8) char lds[(ND * 8 + NI * 4) * WAVE_THREADS];
    double (*red)[WAVE_THREADS] = reinterpret_cast<double (*)[WAVE_THREADS]>(lds);
    int (*cnt)[WAVE_THREADS] = reinterpret_cast<int (*)[WAVE_THREADS]>(lds + ND * 8 * WAVE_THREADS);
    const int tid = threadIdx.x;
    for (int k = 0; k < ND; ++k) red[k][tid] = q[k];
    for (int k = 0; k < NI; ++k) cnt[k][tid] = c[k];
    __syncthreads();
    for (int w = WAVE_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            for (int k = 0; k < ND; ++k) red[k][tid] = op(red[k][tid], red[k][tid + w]);
            for (int k = 0; k < NI; ++k) cnt[k][tid] += cnt[k][tid + w];
        }
        __syncthreads();
    }
    for (int k = 0; k < ND; ++k) q[k] = red[k][0];
    for (int k = 0; k < NI; ++k) c[k] = cnt[k][0];
}

// first[f], f < nf <= WAVE_THREADS: the first sample of frame g0 + f of the call (index over SJ[n], clamped to the last frame:
// total >= 1) -- one search per frame, not one per item: each is a chain of loads.  The caller's barrier publishes it.
__device__ __forceinline__ void frame_first(const EvalArgs &a, int64_t *first, int g0, int nf, int total)
{
    const int f = threadIdx.x;
    if (f < nf) {
        const int g = g0 + f < total ? g0 + f : total - 1, s = sentence_of(a.SJ, a.n, g);
        first[f] = a.off[s] + (int64_t)(g - a.SJ[s]) * a.skip;
    }
}

}  // namespace

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_resample(const EvalArgs a)
{
    const int sg = blockIdx.y, s = sentence_of(a.rb, a.n, blockIdx.x);
    const int k = (blockIdx.x - a.rb[s]) * WAVE_THREADS + threadIdx.x;
    if (k >= a.o10[s + 1] - a.o10[s]) return;
    const float *x = a.sig[sg] + a.off[s];
    const int64_t n = a.len[s], t0 = (int64_t)k * a.q + a.Lh;      // u index at tap 0: u[t] = x[t / p] when p | t, 0 <= t / p < n
    int64_t j = t0 % a.p, i = (t0 - j) / a.p;                       // taps j, j + p, ... meet samples i, i - 1, ...
    if (i >= n) { j += (i - n + 1) * a.p; i = n - 1; }
    double acc = 0.0;
    for (; j < a.taps && i >= 0; j += a.p, --i) acc += (double)a.h[j] * (double)x[i];
    a.r10[sg * a.s10 + a.o10[s] + k] = (float)acc;
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_energy(const EvalArgs a)
{
    const int s = sentence_of(a.eb, a.n, blockIdx.x), ln = threadIdx.x & 63;
    const int j = (blockIdx.x - a.eb[s]) * (WAVE_THREADS / 64) + (threadIdx.x >> 6);
    if (j >= a.P[s + 1] - a.P[s]) return;                           // (a whole wave64: no barrier below)
    const float *x = a.r10 + a.o10[s] + (size_t)j * EV_K;
    double e = 0.0;
    for (int i = ln; i < EV_N; i += 64) { const double u = (double)a.v[i] * (double)x[i]; e += u * u; }
    e = wave_sum(e);
    if (ln == 0) a.E[a.P[s] + j] = e;
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_mask(const EvalArgs a)
{
    __shared__ int cnt[WAVE_THREADS];
    const int s = blockIdx.x, tid = threadIdx.x, base = a.P[s], J = a.P[s + 1] - base;
    double m = 0.0;
    for (int j = tid; j < J; j += WAVE_THREADS) m = fmax(m, a.E[base + j]);
    block_reduce<1, 0>(&m, nullptr, OpMax());
    const double thr = 1e-4 * m;
    int total = 0;
    for (int j0 = 0; j0 < J; j0 += WAVE_THREADS) {
        const int j = j0 + tid, keep = j < J && a.E[base + j] > thr;
        cnt[tid] = keep;
        __syncthreads();
        for (int o = 1; o < WAVE_THREADS; o <<= 1) {                // inclusive scan
            const int add = tid >= o ? cnt[tid - o] : 0;
            __syncthreads();
            cnt[tid] += add;
            __syncthreads();
        }
        if (keep) a.frm[base + total + cnt[tid] - 1] = j;
        total += cnt[WAVE_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) a.C[s] = total;
}

// compacted sample t of a sentence: kept frames c0 = t/K - 1 and c1 = t/K overlap it (c < C)
__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_compact(const EvalArgs a)
{
    const int sg = blockIdx.y, s = sentence_of(a.qb, a.n, blockIdx.x);
    const int t = (blockIdx.x - a.qb[s]) * WAVE_THREADS + threadIdx.x, C = a.C[s], c1 = t / EV_K, c0 = c1 - 1;
    const float *x = a.r10 + sg * a.s10 + a.o10[s];
    const int *frm = a.frm + a.P[s];
    float y = 0.0f;
    if (c0 >= 0 && c0 < C) y = a.v[t - c0 * EV_K] * x[(size_t)frm[c0] * EV_K + t - c0 * EV_K];
    if (c1 < C) y += a.v[t - c1 * EV_K] * x[(size_t)frm[c1] * EV_K + t - c1 * EV_K];
    a.comp[sg * a.scomp + a.Q[s] + t] = y;
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_bands(const EvalArgs a)
{
    extern __shared__ float2 z[];
    const int sg = blockIdx.y, g = blockIdx.x, s = sentence_of(a.P, a.n, g), f = g - a.P[s], tid = threadIdx.x;
    if (f >= a.C[s] - 1) return;                                    // S = C - 1 frames (the grid is sized by the bound)
    float *pw = reinterpret_cast<float *>(z + lds_bytes(1 << EV_LOG2M) / sizeof(float2));   // |X_k|^2 of the band bins
    rfft_frame(z, a.comp + sg * a.scomp + a.Q[s] + (size_t)f * EV_K, a.v, a.tw, EV_LOG2M);
    for (int k = EV_BIN_LO + tid; k < EV_BIN_HI; k += blockDim.x) {
        const float2 X = rfft_bin(z, a.tw, 1 << EV_LOG2M, k);
        pw[k - EV_BIN_LO] = X.x * X.x + X.y * X.y;
    }
    __syncthreads();
    if (tid < EV_NB) {
        double acc = 0.0;
        for (int k = ev_band_lo[tid]; k < ev_band_hi[tid]; ++k) acc += (double)pw[k - EV_BIN_LO];
        a.band[sg * a.sband + (size_t)g * EV_BS + tid] = (float)sqrt(acc);
    }
}

// pair i of a sentence: segment m = 29 + i / 15 (its last frame), band i % 15
__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_corr(const EvalArgs a)
{
    const int e = blockIdx.y + 1, s = sentence_of(a.cb, a.n, blockIdx.x);
    const int i = (blockIdx.x - a.cb[s]) * WAVE_THREADS + threadIdx.x, m = EV_SEG - 1 + i / EV_NB, b = i % EV_NB;
    if (m >= a.C[s] - 1) return;
    const float *X = a.band + (size_t)(a.P[s] + m - (EV_SEG - 1)) * EV_BS + b, *Y = X + e * a.sband;
    double sx = 0.0, sy = 0.0;
    for (int u = 0; u < EV_SEG; ++u) { const double x = X[u * EV_BS], y = Y[u * EV_BS]; sx += x * x; sy += y * y; }
    const double al = sqrt(sx / (sy + EV_EPS));
    double mx = 0.0, my = 0.0;
    for (int u = 0; u < EV_SEG; ++u) { const double x = X[u * EV_BS]; mx += x; my += fmin(al * (double)Y[u * EV_BS], a.clip * x); }
    mx /= EV_SEG; my /= EV_SEG;
    double sxy = 0.0, sxx = 0.0, syy = 0.0;
    for (int u = 0; u < EV_SEG; ++u) {
        const double x = X[u * EV_BS], dx = x - mx, dy = fmin(al * (double)Y[u * EV_BS], a.clip * x) - my;
        sxy += dx * dy; sxx += dx * dx; syy += dy * dy;
    }
    a.rho[(e - 1) * a.srho + a.CP[s] + i] = sxy / ((sqrt(sxx) + EV_EPS) * (sqrt(syy) + EV_EPS));
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_ssnr(const EvalArgs a)
{
    const int e = blockIdx.y + 1, s = sentence_of(a.sb, a.n, blockIdx.x), ln = threadIdx.x & 63;
    const int j = (blockIdx.x - a.sb[s]) * (WAVE_THREADS / 64) + (threadIdx.x >> 6);
    if (j >= a.SJ[s + 1] - a.SJ[s]) return;
    const size_t at = (size_t)a.off[s] + (size_t)j * a.skip;
    const float *r = a.sig[0] + at, *x = a.sig[e] + at;
    double es = 0.0, ed = 0.0;
    for (int i = ln; i < a.win; i += 64) {
        const double rv = r[i], wr = a.w[i] * rv, wd = a.w[i] * (rv - (double)x[i]);
        es += wr * wr; ed += wd * wd;
    }
    es = wave_sum(es); ed = wave_sum(ed);
    if (ln == 0) a.ssnr[(e - 1) * a.sssnr + a.SJ[s] + j] = fmin(fmax(10.0 * log10(es / (ed + EV_EPS) + EV_EPS), -10.0), 35.0);
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_lsd(const EvalArgs a)
{
    const int e = blockIdx.y + 1, ln = threadIdx.x & 63, g = blockIdx.x * (WAVE_THREADS / 64) + (threadIdx.x >> 6);
    if (g >= a.F[a.n]) return;
    const float *lr = a.lps[0] + (size_t)g * a.D, *le = a.lps[e] + (size_t)g * a.D;
    const double db = 4.3429448190325182765;                        // 10 / ln 10
    double acc = 0.0;
    for (int k = ln; k < a.D; k += 64) { const double d = db * ((double)lr[k] - (double)le[k]); acc += d * d; }
    acc = wave_sum(acc);
    if (ln == 0) a.lsd[(e - 1) * a.slsd + g] = sqrt(acc / a.D);
}

// segment g of the call (CP / 15 is the segment prefix): m = 29 + g - CP[s] / 15 is its last frame; signal k's matrix lies in
// LDS as mat[k][u][b] with a row of EV_MS doubles per frame u (17: the column step's stride of 34 banks meets every bank pair once)
constexpr int EV_MS = 17, EV_MAT = EV_SEG * EV_MS;
__global__ __launch_bounds__(64) void bp_eval_estoi(const EvalArgs a)
{
    __shared__ double mat[EVAL_MAXSIG * EV_MAT];
    const int g = blockIdx.x, s = sentence_of(a.CP, a.n, EV_NB * g), i = g - a.CP[s] / EV_NB, ln = threadIdx.x;
    if (i + EV_SEG - 1 >= a.C[s] - 1) return;                       // (the whole wave64: the barriers below are met by all or none)
    const float *X = a.band + (size_t)(a.P[s] + i) * EV_BS;
    for (int t = ln; t < a.nsig * EV_SEG * EV_BS; t += 64) {
        const int k = t / (EV_SEG * EV_BS), r = t % (EV_SEG * EV_BS), u = r / EV_BS, b = r % EV_BS;
        if (b < EV_NB) mat[k * EV_MAT + u * EV_MS + b] = (double)X[k * a.sband + r];
    }
    __syncthreads();
    for (int t = ln; t < a.nsig * EV_NB; t += 64) {                 // rows: band b of signal k over the 30 frames
        double *x = mat + (t / EV_NB) * EV_MAT + t % EV_NB;
        double m = 0.0, q = 0.0;
        for (int u = 0; u < EV_SEG; ++u) m += x[u * EV_MS];
        m /= EV_SEG;
        for (int u = 0; u < EV_SEG; ++u) { const double d = x[u * EV_MS] - m; x[u * EV_MS] = d; q += d * d; }
        q = sqrt(q) + EV_EPS;
        for (int u = 0; u < EV_SEG; ++u) x[u * EV_MS] /= q;
    }
    __syncthreads();
    for (int t = ln; t < a.nsig * EV_SEG; t += 64) {                // columns: frame u of signal k over the 15 bands
        double *x = mat + (t / EV_SEG) * EV_MAT + (t % EV_SEG) * EV_MS;
        double m = 0.0, q = 0.0;
        for (int b = 0; b < EV_NB; ++b) m += x[b];
        m /= EV_NB;
        for (int b = 0; b < EV_NB; ++b) { const double d = x[b] - m; x[b] = d; q += d * d; }
        q = sqrt(q) + EV_EPS;
        for (int b = 0; b < EV_NB; ++b) x[b] /= q;
    }
    __syncthreads();
    for (int e = 1; e < a.nsig; ++e) {
        double d = 0.0;
        for (int t = ln; t < EV_SEG * EV_NB; t += 64) {
            const int at = (t / EV_NB) * EV_MS + t % EV_NB;
            d += mat[at] * mat[e * EV_MAT + at];
        }
        d = wave_sum(d);
        if (ln == 0) a.dm[(e - 1) * a.sdm + a.CP[s] / EV_NB + i] = d / EV_SEG;
    }
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_sisdr(const EvalArgs a)
{
    const int s = blockIdx.x, e = blockIdx.y + 1, tid = threadIdx.x, n = a.len[s];
    const float *r = a.sig[0] + a.off[s], *x = a.sig[e] + a.off[s];
    double q[2] = {0.0, 0.0}, p[2] = {0.0, 0.0};                    // rr, er; then num, den (the residual itself, no cancellation)
    for (int i = tid; i < n; i += WAVE_THREADS) {
        const double rv = r[i], xv = x[i];
        q[0] += rv * rv; q[1] += xv * rv;
    }
    block_reduce<2, 0>(q, nullptr);
    __syncthreads();                                                // (read before the second pass writes the LDS again)
    if (q[0] == 0.0) {                                              // a silent reference (uniform over the workgroup)
        if (tid == 0) a.sdr[(size_t)(e - 1) * a.n + s] = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const double al = q[1] / q[0];
    for (int i = tid; i < n; i += WAVE_THREADS) {
        const double rv = r[i], xv = x[i], t = al * rv, d = t - xv;
        p[0] += t * t; p[1] += d * d;
    }
    block_reduce<2, 0>(p, nullptr);
    if (tid == 0) a.sdr[(size_t)(e - 1) * a.n + s] = 10.0 * log10(p[0] / (p[1] + EV_EPS) + EV_EPS);
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_reduce(const EvalArgs a)
{
    const int s = blockIdx.x, e = blockIdx.y + 1, tid = threadIdx.x;
    const int J = a.SJ[s + 1] - a.SJ[s], T = a.F[s + 1] - a.F[s], S = a.C[s] - 1, np = S >= EV_SEG ? EV_NB * (S - (EV_SEG - 1)) : 0;
    const double *ss = a.ssnr + (e - 1) * a.sssnr + a.SJ[s], *ls = a.lsd + (e - 1) * a.slsd + a.F[s], *rh = a.rho + (e - 1) * a.srho + a.CP[s];
    const bool ext = a.ns >= BP_SCORE_EXT_N;
    const int nd = ext ? np / EV_NB : 0;                            // the S - 29 segments
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < J; i += WAVE_THREADS) q[0] += ss[i];
    for (int i = tid; i < T; i += WAVE_THREADS) q[1] += ls[i];
    for (int i = tid; i < np; i += WAVE_THREADS) q[2] += rh[i];
    for (int i = tid; i < nd; i += WAVE_THREADS) q[3] += a.dm[(e - 1) * a.sdm + a.CP[s] / EV_NB + i];
    block_reduce<4, 0>(q, nullptr);
    if (tid == 0) {
        float *o = a.scores + ((size_t)(e - 1) * a.n + s) * a.ns;
        o[BP_SCORE_SSNR] = J >= 1 ? (float)(q[0] / J) : EV_NAN;
        o[BP_SCORE_LSD] = T >= 1 ? (float)(q[1] / T) : EV_NAN;
        o[BP_SCORE_STOI] = np > 0 ? (float)(q[2] / np) : EV_NAN;
        if (ext) {
            o[BP_SCORE_ESTOI] = nd > 0 ? (float)(q[3] / nd) : EV_NAN;
            o[BP_SCORE_SISDR] = (float)a.sdr[(size_t)(e - 1) * a.n + s];
        }
    }
}

// ---- LLR and cepstral distance (seven columns).  EV_LPAD zeros behind each windowed frame in LDS let every lag sum run over all
// win samples: the products past the end are exact zeros.  A wave64 sums the lags of one frame as 4 lag groups x 16 sample
// segments: lane (group, segment) keeps the EV_LL(P) lags from group EV_LL(P) on, over the samples i = segment (mod 16).
constexpr int EV_LPAD = 24;
__host__ __device__ constexpr int EV_LL(int P) { return (P + 4) / 4; }   // lags per lane: 3 (P = 10), 5 (P = 16); 4 EV_LL(P) - 1 < EV_LPAD
constexpr double EV_WNC = 1.0 + 1e-6;                               // the white-noise correction of R[0]

// Levinson-Durbin on R (R[0] corrected) and the LPC cepstrum: a[1..P], c[1..P] (index 0 unused).  Fully unrolled: registers only.
template <int P> __device__ __forceinline__ void lpc_of(const double (&R)[P + 1], double (&a)[P + 1], double (&c)[P + 1])
{
    double E = R[0];
#pragma unroll
    for (int m = 1; m <= P; ++m) {
        double sum = 0.0;
#pragma unroll
        for (int j = 1; j < m; ++j) sum += a[j] * R[m - j];
        const double k = (R[m] - sum) / E;
#pragma unroll
        for (int j = 1; j < m - j; ++j) {                           // a'[j] = a[j] - k a[m - j], in place by pairs
            const double lo = a[j], hi = a[m - j];
            a[j] = lo - k * hi; a[m - j] = hi - k * lo;
        }
        if (m % 2 == 0) a[m / 2] -= k * a[m / 2];
        a[m] = k;
        E = (1.0 - k * k) * E;
    }
    c[1] = a[1];
#pragma unroll
    for (int m = 2; m <= P; ++m) {
        double sum = 0.0;
#pragma unroll
        for (int q = 1; q < m; ++q) sum += ((double)q / (double)m) * c[q] * a[m - q];
        c[m] = a[m] + sum;
    }
}

// A T A^T with A = [1, -a_1 .. -a_P] and T the Toeplitz matrix of R: rows in order, each row's sum first
template <int P> __device__ __forceinline__ double lpc_form(const double (&a)[P + 1], const double (&R)[P + 1])
{
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i <= P; ++i) {
        double row = 0.0;
#pragma unroll
        for (int j = 0; j <= P; ++j) row += (j == 0 ? 1.0 : -a[j]) * R[i > j ? i - j : j - i];
        tot += (i == 0 ? 1.0 : -a[i]) * row;
    }
    return tot;
}

// Frame block of bp_eval_lpc: EV_FB consecutive frames of the call (global index g over SJ[n]; a block may span sentences).
// LDS, in doubles: one slab of win + EV_LPAD per wave (the windowed frame; only up to EV_SLAB_WIN samples -- above that the lag
// sums read the samples again from memory), Rl[signal][lag][frame], then Cr[m][frame] and Dl[frame] of the reference.
constexpr int EV_FB = 32, EV_SLAB_WIN = 1440, EV_LB = 8;
__host__ __device__ constexpr size_t lpc_slab_doubles(int win) { return win <= EV_SLAB_WIN ? (size_t)(WAVE_THREADS / 64) * (win + EV_LPAD) : 0; }

// the lags k0 .. k0 + EV_LL(P) - 1 of the windowed frame at x, k0 = (lane / 16) EV_LL(P), in every lane of the group: each lane's
// sum over its samples in order, then a fixed shuffle tree over the 16 segments (the barriers are met by the whole workgroup)
template <int P> __device__ __forceinline__ void lpc_lags(const EvalArgs &a, const float *__restrict__ x, bool live, double *xw, int ln,
                                                          double (&R)[EV_LL(P)])
{
    constexpr int L = EV_LL(P);
    const bool slab = a.win <= EV_SLAB_WIN;
    const double *__restrict__ w = a.w;
    const int sgm = ln & 15, k0 = (ln >> 4) * L;
    if (slab) {
        if (live)
            for (int i0 = ln; i0 < a.win; i0 += 64 * EV_LB) {       // EV_LB loads of either table in flight, then the products
                float xv[EV_LB];
                double wv[EV_LB];
#pragma unroll
                for (int u = 0; u < EV_LB; ++u) {
                    const int i = i0 + 64 * u < a.win ? i0 + 64 * u : a.win - 1;
                    xv[u] = x[i]; wv[u] = w[i];
                }
#pragma unroll
                for (int u = 0; u < EV_LB; ++u)
                    if (i0 + 64 * u < a.win) xw[i0 + 64 * u] = wv[u] * (double)xv[u];
            }
        __syncthreads();
    }
#pragma unroll
    for (int l = 0; l < L; ++l) R[l] = 0.0;
    if (live && slab)
        for (int i = sgm; i < a.win; i += 16) {
            const double x0 = xw[i];
#pragma unroll
            for (int l = 0; l < L; ++l) R[l] += x0 * xw[i + k0 + l];
        }
    if (live && !slab)
        for (int i = sgm; i < a.win; i += 16) {
            const double x0 = w[i] * (double)x[i];
#pragma unroll
            for (int l = 0; l < L; ++l)
                if (i + k0 + l < a.win) R[l] += x0 * (w[i + k0 + l] * (double)x[i + k0 + l]);
        }
    if (slab) __syncthreads();
#pragma unroll
    for (int l = 0; l < L; ++l)
        for (int o = 8; o > 0; o >>= 1) R[l] += __shfl_xor(R[l], o);
}

template <int P> __global__ __launch_bounds__(WAVE_THREADS) void bp_eval_lpc(const EvalArgs a)
{
    extern __shared__ double lpc_lds[];
    __shared__ int64_t first[EV_FB];                                // the first sample of each frame of the block
    const int tid = threadIdx.x, ln = tid & 63, wv = tid >> 6, g0 = blockIdx.x * EV_FB, total = a.SJ[a.n];
    frame_first(a, first, g0, EV_FB, total);
    double *xw = lpc_lds + (size_t)wv * (a.win + EV_LPAD);
    double *Rl = lpc_lds + lpc_slab_doubles(a.win), *Cr = Rl + (size_t)a.nsig * (P + 1) * EV_FB, *Dl = Cr + (size_t)P * EV_FB;
    if (a.win <= EV_SLAB_WIN && ln < EV_LPAD) xw[a.win + ln] = 0.0;
    __syncthreads();
    // 1. the lags: item t = (signal t / EV_FB, frame t % EV_FB) of the block, one wave64 each, the waves taking the items in turn
    for (int t = wv; t < a.nsig * EV_FB; t += WAVE_THREADS / 64) {  // (the same number of rounds in every wave: EV_FB % 4 == 0)
        const int k = t / EV_FB, f = t % EV_FB;
        const bool live = g0 + f < total;
        const float *x = a.sig[k] + first[f];
        double R[EV_LL(P)];
        lpc_lags<P>(a, x, live, xw, ln, R);
        if ((ln & 15) == 0) {
#pragma unroll
            for (int l = 0; l < EV_LL(P); ++l) {
                const int q = (ln >> 4) * EV_LL(P) + l;
                if (q <= P) Rl[((size_t)k * (P + 1) + q) * EV_FB + f] = R[l];
            }
        }
    }
    __syncthreads();
    // 2. the recursions: thread t = (signal, frame) as above; the reference's cepstrum and quadratic form go to LDS
    const int k = tid / EV_FB, f = tid % EV_FB, g = g0 + f;
    const bool work = tid < a.nsig * EV_FB && g < total;
    double R[P + 1], al[P + 1], c[P + 1];
    bool pos = false;
    if (work) {                                                     // (the waves past nsig EV_FB threads skip it whole)
#pragma unroll
        for (int q = 0; q <= P; ++q) R[q] = Rl[((size_t)k * (P + 1) + q) * EV_FB + f];
        pos = R[0] > 0.0;
        R[0] *= EV_WNC;
        lpc_of<P>(R, al, c);
        if (k == 0) {
#pragma unroll
            for (int m = 1; m <= P; ++m) Cr[(size_t)(m - 1) * EV_FB + f] = c[m];
            Dl[f] = lpc_form<P>(al, R);
        }
    }
    __syncthreads();
    if (work && k > 0) {
        double Rr[P + 1], d2 = 0.0;
#pragma unroll
        for (int q = 0; q <= P; ++q) Rr[q] = Rl[(size_t)q * EV_FB + f];
        const bool valid = pos && Rr[0] > 0.0;
        Rr[0] *= EV_WNC;
        const double num = lpc_form<P>(al, Rr);
#pragma unroll
        for (int m = 1; m <= P; ++m) { const double d = Cr[(size_t)(m - 1) * EV_FB + f] - c[m]; d2 += d * d; }
        const size_t o = (size_t)(k - 1) * a.sssnr + g;
        a.llr[o] = valid ? fmin(fmax(log(num / Dl[f]), 0.0), 2.0) : 0.0;
        a.lcd[o] = valid ? fmin(fmax(4.3429448190325182765 * sqrt(2.0 * d2), 0.0), 10.0) : 0.0;
        a.lv[o] = valid;
    }
}

// Jk of Jv valid frames: the lowest 95 %, at least one
__device__ __forceinline__ int lpc_keep(int Jv) { const int k = (int)floor(0.95 * (double)Jv + 0.5); return k > 1 ? k : 1; }

// Rank-and-select over the NV value arrays of a.rank.  One thread per frame (global index g; a block may span sentences): the
// values of all the sentences the block touches pass through LDS in tiles, and every thread counts the frames of its own sentence
// among them (the reads of a tile entry are the same address in every lane)
template <int NV> __device__ __forceinline__ void rank_select(const EvalArgs &a, double (*tx)[WAVE_THREADS], int *tv)
{
    const RankSel &r = a.rank;
    const int e = blockIdx.y + 1, tid = threadIdx.x, total = a.SJ[a.n], g0 = blockIdx.x * WAVE_THREADS;
    const int glast = g0 + WAVE_THREADS - 1 < total ? g0 + WAVE_THREADS - 1 : total - 1, g = g0 + tid;
    const bool live = g < total;
    const int s = sentence_of(a.SJ, a.n, live ? g : glast), lo = a.SJ[s], hi = a.SJ[s + 1];
    const int ulo = a.SJ[sentence_of(a.SJ, a.n, g0)], uhi = a.SJ[sentence_of(a.SJ, a.n, glast) + 1];   // (uniform over the workgroup)
    const size_t o = (size_t)(e - 1) * a.sssnr;
    double xj[NV];
    int jv = 0, rk[NV];                                             // valid frames; frames ranked before g in each measure
    for (int k = 0; k < NV; ++k) { xj[k] = live ? r.val[k][o + g] : 0.0; rk[k] = 0; }
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    for (int t0 = ulo; t0 < uhi; t0 += WAVE_THREADS) {
        const int i = t0 + tid, m = uhi - t0 < WAVE_THREADS ? uhi - t0 : WAVE_THREADS;
        if (i < uhi) {                                              // (an invalid frame is +inf here: below no frame, equal to no valid one)
            const int v = r.valid[o + i];
            for (int k = 0; k < NV; ++k) tx[k][tid] = v ? r.val[k][o + i] : inf;
            tv[tid] = v;
        }
        __syncthreads();
        // the thread's own sentence within the tile: the frames before g count when not above, the frames behind g when below
        const int u0 = lo > t0 ? lo - t0 : 0, u3 = hi - t0 < m ? hi - t0 : m;
        const int u1 = g - t0 < u3 ? g - t0 : u3, u2 = g + 1 - t0 > u0 ? g + 1 - t0 : u0;
        for (int u = u0; u < u1; ++u) {
            jv += tv[u];
            for (int k = 0; k < NV; ++k) rk[k] += tx[k][u] <= xj[k];
        }
        for (int u = u2; u < u3; ++u) {
            jv += tv[u];
            for (int k = 0; k < NV; ++k) rk[k] += tx[k][u] < xj[k];
        }
        if (g >= t0 && g < t0 + m) jv += tv[g - t0];
        __syncthreads();
    }
    if (live) {
        const int Jk = lpc_keep(jv);
        int sel = 0;
        for (int k = 0; k < NV; ++k) sel |= rk[k] < Jk ? 1 << k : 0;
        r.sel[o + g] = r.valid[o + g] ? sel : 0;
    }
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_lpcrank(const EvalArgs a)
{
    __shared__ double tx[2][WAVE_THREADS];
    __shared__ int tv[WAVE_THREADS];
    if (a.rank.nval == 2) rank_select<2>(a, tx, tv);
    else rank_select<1>(a, tx, tv);
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_lpcsum(const EvalArgs a)
{
    const int s = blockIdx.x, e = blockIdx.y + 1, tid = threadIdx.x, J = a.SJ[s + 1] - a.SJ[s];
    const size_t o = (size_t)(e - 1) * a.sssnr + a.SJ[s];
    double q[2] = {0.0, 0.0};
    int Jv = 0;
    for (int i = tid; i < J; i += WAVE_THREADS) {
        const int sel = a.lsel[o + i];
        Jv += a.lv[o + i];
        if (sel & 1) q[0] += a.llr[o + i];
        if (sel & 2) q[1] += a.lcd[o + i];
    }
    block_reduce<2, 1>(q, &Jv);
    if (tid == 0) {
        float *sc = a.scores + ((size_t)(e - 1) * a.n + s) * a.ns;
        const int Jk = lpc_keep(Jv);
        sc[BP_SCORE_LLR] = Jv > 0 ? (float)(q[0] / Jk) : EV_NAN;
        sc[BP_SCORE_CD] = Jv > 0 ? (float)(q[1] / Jk) : EV_NAN;
    }
}

// ---- fwSegSNR and WSS (nine columns).  Frame block of bp_eval_cb: EV_CF consecutive frames of the call (global index g over
// SJ[n]; a block may span sentences).  The workgroup transforms G = 256 / T (signal, frame) items at a time, T = cb_threads(H)
// threads each: a thread has at least two butterflies per stage, and at 80 kHz, where the points of one item are 68 KB, the
// whole workgroup takes one item.  LDS, in doubles: per item in flight its H = n_fft / 2 complex points (one point of padding
// after every 16: a point is 16 bytes, 16 of them fill the 64 banks once), then bs[signal][band][frame] = (c or d, B or C) and
// ok[signal][frame].
constexpr int EV_CBN = 25, EV_CF = 16;
__device__ __forceinline__ int lpd(int i) { return i + (i >> 4); }
__host__ __device__ constexpr int cb_threads(int H) { return H / 4 < 64 ? 64 : H / 4 > WAVE_THREADS ? WAVE_THREADS : H / 4; }
__host__ __device__ constexpr size_t cb_z_doubles(int H) { return 2 * (size_t)(H + H / 16 + 1); }
__host__ __device__ constexpr size_t cb_lds_bytes(int H, int nsig)
{
    return ((size_t)(WAVE_THREADS / cb_threads(H)) * cb_z_doubles(H) + (size_t)nsig * EV_CBN * EV_CF * 2) * 8 + (size_t)nsig * EV_CF * 4;
}

// the nearest peak of band i in the dB band energies B[0], B[st], .. B[24 st] (the search of the header, step for step)
__device__ __forceinline__ double cb_peak(const double *B, int st, int i)
{
    int n = i;
    if (B[(i + 1) * st] - B[i * st] > 0.0) {
        while (n < EV_CBN - 1 && B[(n + 1) * st] - B[n * st] > 0.0) ++n;
        return B[(n - 1) * st];
    }
    while (n >= 0 && B[(n + 1) * st] - B[n * st] <= 0.0) --n;
    return B[(n + 1) * st];
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_cb(const EvalArgs a)
{
    extern __shared__ __align__(16) double cb_lds[];
    __shared__ int64_t first[EV_CF];
    __shared__ double part[WAVE_THREADS / 64];
    __shared__ int wnz[WAVE_THREADS / 64];
    const int tid = threadIdx.x, ln = tid & 63, wv = tid >> 6, g0 = blockIdx.x * EV_CF, total = a.SJ[a.n], H = a.cH;
    const int nf = total - g0 < EV_CF ? total - g0 : EV_CF;         // frames of this block (>= 1: the grid is sized by total)
    const int T = cb_threads(H), G = WAVE_THREADS / T, slot = tid / T, lt = tid % T, wps = T / 64, L = T / 32;
    int log2H = 0;
    while ((1 << log2H) < H) ++log2H;
    frame_first(a, first, g0, nf, total);
    double2 *z = reinterpret_cast<double2 *>(cb_lds) + (size_t)slot * (cb_z_doubles(H) / 2);
    double2 *bs = reinterpret_cast<double2 *>(cb_lds + (size_t)G * cb_z_doubles(H));
    int *ok = reinterpret_cast<int *>(bs + (size_t)a.nsig * EV_CBN * EV_CF);
    __syncthreads();
    // 1. the items t = (signal t / nf, frame t % nf), G per round, item t0 + slot by the T threads of its slot (every barrier is
    // met by the whole workgroup; what a slot does between them depends on its own item alone)
    for (int t0 = 0; t0 < a.nsig * nf; t0 += G) {
        const int t = t0 + slot, k = t / nf, f = t % nf;
        const bool item = t < a.nsig * nf;
        // the windowed frame as H complex points z[m] = (xw[2m], xw[2m+1]), zeros from win on, at bit-reversed places.  Valid iff
        // sum (w x)^2 > 0: w > 0 throughout and no such product or square underflows, so iff any sample is not zero
        int nz = 0;
        if (item) {
            const float *__restrict__ x = a.sig[k] + first[f];
            for (int m = lt; m < H; m += T) {
                double re = 0.0, im = 0.0;
                if (2 * m < a.win) { const float v = x[2 * m]; nz |= v != 0.0f; re = a.w[2 * m] * (double)v; }
                if (2 * m + 1 < a.win) { const float v = x[2 * m + 1]; nz |= v != 0.0f; im = a.w[2 * m + 1] * (double)v; }
                z[lpd((int)(__brev((unsigned)m) >> (32 - log2H)))] = make_double2(re, im);
            }
        }
        nz = __any(nz);
        if (ln == 0) wnz[wv] = nz;
        __syncthreads();
        bool live = false;
        for (int u = 0; u < wps; ++u) live |= wnz[slot * wps + u] != 0;
        live &= item;
        if (item && lt == 0) ok[k * EV_CF + f] = live;
        for (int h = 1; h < H; h <<= 1) {                            // radix-2 decimation in time, as fft_lds
            const int tstep = H / h;
            if (live)
                for (int j = lt; j < H / 2; j += T) {
                    const int jh = j & (h - 1), i0 = ((j - jh) << 1) + jh, i1 = i0 + h;
                    const double2 w = a.ctw[jh * tstep], p = z[lpd(i0)], q = z[lpd(i1)];
                    const double bx = q.x * w.x - q.y * w.y, by = q.x * w.y + q.y * w.x;
                    z[lpd(i0)] = make_double2(p.x + bx, p.y + by);
                    z[lpd(i1)] = make_double2(p.x - bx, p.y - by);
                }
            __syncthreads();
        }
        // split step in place, the pair (k2, H - k2) by one thread: X[k2] = E + W^k2 O and |X[H - k2]| = |E - W^k2 O|;
        // z[k2] <- (|X|, |X|^2)
        if (live)
            for (int k2 = lt; k2 <= H / 2; k2 += T) {
                const int m = (H - k2) & (H - 1);
                const double2 zk = z[lpd(k2)], zm = z[lpd(m)], w = a.ctw[k2];
                const double ex = 0.5 * (zk.x + zm.x), ey = 0.5 * (zk.y - zm.y), ox = 0.5 * (zk.y + zm.y), oy = -0.5 * (zk.x - zm.x);
                const double tx = ox * w.x - oy * w.y, ty = ox * w.y + oy * w.x;
                const double p0 = (ex + tx) * (ex + tx) + (ey + ty) * (ey + ty), p1 = (ex - tx) * (ex - tx) + (ey - ty) * (ey - ty);
                z[lpd(k2)] = make_double2(sqrt(p0), p0);
                if (m != k2) z[lpd(m)] = make_double2(sqrt(p1), p1);
            }
        __syncthreads();
        double tot = 0.0;                                           // sum |X|: each thread's bins in order, a fixed tree over the threads
        if (live)
            for (int k2 = lt; k2 < H; k2 += T) tot += z[lpd(k2)].x;
        tot = wave_sum(tot);
        if (ln == 0) part[wv] = tot;
        // the band sums: band lt / L by L = T / 32 lanes, each lane's bins in order, a fixed tree over the L
        const int i = lt / L, sub = lt % L;
        double sm = 0.0, sp = 0.0;
        if (live && i < EV_CBN) {
            const int b0 = a.cband[i], cnt = a.cband[EV_CBN + i];
            const double *__restrict__ gw = a.cg + a.cband[2 * EV_CBN + i];
            for (int q = sub; q < cnt; q += L) { const double2 v = z[lpd(b0 + q)]; sm += gw[q] * v.x; sp += gw[q] * v.y; }
        }
        for (int o = L >> 1; o > 0; o >>= 1) { sm += __shfl_xor(sm, o); sp += __shfl_xor(sp, o); }
        __syncthreads();
        if (live && i < EV_CBN && sub == 0) {
            double all = part[slot * wps];                          // (the slot's waves in order)
            for (int u = 1; u < wps; ++u) all += part[slot * wps + u];
            bs[((size_t)k * EV_CBN + i) * EV_CF + f] = make_double2(sm / all, 10.0 * log10(fmax(sp, 1e-10)));
        }
        __syncthreads();                                            // (part, wnz and z are free for the next round)
    }
    // 2. the 25-band part: 32 lanes per (estimate, frame), lane i < 25 on band i (its power, its two logarithms and its two peak
    // searches are where the time of this part goes), the four sums over the bands by a fixed shuffle tree over the 32
    const int np = (a.nsig - 1) * nf, i = tid & 31;
    for (int p0 = 0; p0 < np; p0 += WAVE_THREADS / 32) {
        const int p = p0 + (tid >> 5), e = p / nf + 1, f = p % nf;
        const bool pair = p < np, valid = pair && ok[f] && ok[e * EV_CF + f];
        double fn = 0.0, fd = 0.0, wn = 0.0, wd = 0.0, bmax = -1e300, cmax = -1e300;
        const double2 *R = bs + f, *E = bs + (size_t)e * EV_CBN * EV_CF + f;   // band i at [i EV_CF]
        const double *B = &R[0].y, *C = &E[0].y;                    // stride 2 EV_CF doubles per band
        constexpr int st = 2 * EV_CF;
        const bool on = valid && i < EV_CBN;
        if (on) {
            const double c = R[i * EV_CF].x, d = E[i * EV_CF].x;
            if (c > 0.0) {
                const double df = c - d, err = fmax(df * df, EV_EPS);
                fd = pow(c, 0.2);
                fn = fd * (10.0 * log10(c * c / err));
            }
            bmax = B[i * st]; cmax = C[i * st];
        }
        for (int o = 16; o > 0; o >>= 1) { bmax = fmax(bmax, __shfl_xor(bmax, o)); cmax = fmax(cmax, __shfl_xor(cmax, o)); }
        if (on && i < EV_CBN - 1) {
            const double Bi = B[i * st], Ci = C[i * st], s = B[(i + 1) * st] - Bi, u = C[(i + 1) * st] - Ci;
            const double wr = 20.0 / (20.0 + bmax - Bi) * (1.0 / (1.0 + cb_peak(B, st, i) - Bi));
            const double we = 20.0 / (20.0 + cmax - Ci) * (1.0 / (1.0 + cb_peak(C, st, i) - Ci));
            wd = (wr + we) / 2.0;
            wn = wd * ((s - u) * (s - u));
        }
        for (int o = 16; o > 0; o >>= 1) {
            fn += __shfl_xor(fn, o); fd += __shfl_xor(fd, o); wn += __shfl_xor(wn, o); wd += __shfl_xor(wd, o);
        }
        if (pair && i == 0) {
            const bool fok = valid && fd > 0.0;
            const size_t o = (size_t)(e - 1) * a.sssnr + g0 + f;
            a.fw[o] = fok ? fmin(fmax(fn / fd, -10.0), 35.0) : 0.0; a.fv[o] = fok;
            a.ws[o] = valid ? wn / wd : 0.0; a.wv[o] = valid;
        }
    }
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_cbsum(const EvalArgs a)
{
    const int s = blockIdx.x, e = blockIdx.y + 1, tid = threadIdx.x, J = a.SJ[s + 1] - a.SJ[s];
    const size_t o = (size_t)(e - 1) * a.sssnr + a.SJ[s];
    double q[2] = {0.0, 0.0};
    int nv[2] = {0, 0};                                             // valid frames of fwSegSNR, of WSS
    for (int i = tid; i < J; i += WAVE_THREADS) {
        nv[0] += a.fv[o + i]; nv[1] += a.wv[o + i];
        if (a.fv[o + i]) q[0] += a.fw[o + i];
        if (a.csel[o + i] & 1) q[1] += a.ws[o + i];
    }
    block_reduce<2, 2>(q, nv);
    if (tid == 0) {
        float *sc = a.scores + ((size_t)(e - 1) * a.n + s) * a.ns;
        sc[BP_SCORE_FWSSNR] = nv[0] > 0 ? (float)(q[0] / nv[0]) : EV_NAN;
        sc[BP_SCORE_WSS] = nv[1] > 0 ? (float)(q[1] / lpc_keep(nv[1])) : EV_NAN;
    }
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_eval_trim(const int64_t *__restrict__ off, const int *__restrict__ len,
                                                          const int *__restrict__ FS, int n, int hop, float *__restrict__ pcm)
{
    const int q = blockIdx.x, s = sentence_of(FS, n, q);
    for (int r = threadIdx.x; r < hop; r += blockDim.x) {
        const int64_t at = (int64_t)q * hop + r, i = at - off[s];
        if (i < 0 || i >= len[s]) pcm[at] = 0.0f;
    }
}

// ------------------------------------------------------------------ host side
namespace {

// Where the tables lie in the table block (all offsets 256-byte aligned).
struct TabLayout {
    size_t off, len, pre[PRE_N], h, v, tw, w, ctw, cband, cg, bytes;   // pre: the prefix tables by id; c*: EVAL_ALL only
};
TabLayout tab_layout(const EvalPlan &ep)
{
    TabLayout t;
    const size_t n = (size_t)ep.n;
    Layout lay;
    t.off = lay.take(n * 8); t.len = lay.take(n * 4);
    for (int k = 0; k < PRE_N; ++k) t.pre[k] = lay.take((n + 1) * 4);
    t.h = lay.take((size_t)ep.taps * 4);
    t.v = lay.take((size_t)EV_NFFT * 4);
    t.tw = lay.take((size_t)(EV_NFFT / 2 + 1) * 8);
    t.w = lay.take((size_t)ep.win * 8);
    const bool all = ep.has(EVAL_ALL);                              // (a part of 0 bytes takes no room)
    t.ctw = lay.take(all ? (size_t)(ep.cH + 1) * 16 : 0);
    t.cband = lay.take(all ? (size_t)3 * EV_CBN * 4 : 0);
    t.cg = lay.take(all ? ep.cb_g.size() * 8 : 0);
    t.bytes = lay.size();
    return t;
}

double bessel_i0(double x)
{
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 200 && t > 1e-20 * s; ++k) { t *= (x / (2.0 * k)) * (x / (2.0 * k)); s += t; }
    return s;
}

// The work block: one row per array, in block order.  An array holds `per` x extent elements, and the narrowest width that has it
// says whether it takes room (a part of 0 bytes takes none); bind puts its address, and the extent where a kernel strides by it,
// into the argument block.
enum Per { PER_SIG, PER_EST, ONCE };
enum Extent { X_O10, X_P, X_N, X_Q, X_BAND, X_CP, X_SJ, X_F, X_SEG, X_COUNT };   // (X_O10: rounded up to 4 samples)
struct WorkRow { const char *name; void (*bind)(EvalArgs &, char *, size_t); size_t elem; Per per; Extent ext; EvalWidth width; };
#define ROW(p, stride, per, ext, width) \
    {#p, [](EvalArgs &a, char *at, size_t st) { a.p = (decltype(a.p))at; stride; }, sizeof(*EvalArgs().p), per, ext, width}
const WorkRow work_rows[] = {
    ROW(r10, a.s10 = st, PER_SIG, X_O10, EVAL_BASIC),
    ROW(E, (void)st, ONCE, X_P, EVAL_BASIC),
    ROW(frm, (void)st, ONCE, X_P, EVAL_BASIC),
    ROW(C, (void)st, ONCE, X_N, EVAL_BASIC),
    ROW(comp, a.scomp = st, PER_SIG, X_Q, EVAL_BASIC),
    ROW(band, a.sband = st, PER_SIG, X_BAND, EVAL_BASIC),
    ROW(rho, a.srho = st, PER_EST, X_CP, EVAL_BASIC),
    ROW(ssnr, a.sssnr = st, PER_EST, X_SJ, EVAL_BASIC),             // (sssnr: the stride of every [est][SJ[n]] array below)
    ROW(lsd, a.slsd = st, PER_EST, X_F, EVAL_BASIC),
    ROW(dm, a.sdm = st, PER_EST, X_SEG, EVAL_EXT),
    ROW(sdr, (void)st, PER_EST, X_N, EVAL_EXT),
    ROW(llr, (void)st, PER_EST, X_SJ, EVAL_FULL),
    ROW(lcd, (void)st, PER_EST, X_SJ, EVAL_FULL),
    ROW(lv, (void)st, PER_EST, X_SJ, EVAL_FULL),
    ROW(lsel, (void)st, PER_EST, X_SJ, EVAL_FULL),
    ROW(fw, (void)st, PER_EST, X_SJ, EVAL_ALL),
    ROW(ws, (void)st, PER_EST, X_SJ, EVAL_ALL),
    ROW(fv, (void)st, PER_EST, X_SJ, EVAL_ALL),
    ROW(wv, (void)st, PER_EST, X_SJ, EVAL_ALL),
    ROW(csel, (void)st, PER_EST, X_SJ, EVAL_ALL),
};
#undef ROW
// Walks the table: the size of the work block for nsig signals and, with a, the binding of every array at work
size_t work_walk(const EvalPlan &ep, int nsig, EvalArgs *a = nullptr, char *work = nullptr)
{
    const size_t o10 = ep.tot(PRE_o10), P = ep.tot(PRE_P), CP = ep.tot(PRE_CP);
    const size_t extent[X_COUNT] = {(o10 + 3) & ~(size_t)3, P, (size_t)ep.n, (size_t)ep.tot(PRE_Q), P * EV_BS, CP, (size_t)ep.tot(PRE_SJ),
                                    (size_t)ep.tot(PRE_F), CP / EV_NB};
    Layout lay;
    for (const WorkRow &r : work_rows) {
        const size_t ext = extent[r.ext], per = r.per == PER_SIG ? nsig : r.per == PER_EST ? nsig - 1 : 1;
        const size_t at = lay.take(ep.has(r.width) ? per * ext * r.elem : 0);
        if (a) r.bind(*a, work + at, ext);
    }
    return lay.size();
}

}  // namespace

bool eval_rate(int fs, int *p, int *q)
{
    if (fs <= 0) return false;
    int a = 10000, b = fs;
    while (b) { const int t = a % b; a = b; b = t; }
    *p = 10000 / a; *q = fs / a;
    return *p <= 32 && *q <= 32;
}

int eval_n_scores(const char *who, int n_scores)
{
    std::string names;                                             // "A, B, C or D"
    for (int w = 0; w < EVAL_WIDTH_N; ++w) {
        if (n_scores == EVAL_WIDTHS[w].ns) return BP_OK;
        names += std::string(w == 0 ? "" : w == EVAL_WIDTH_N - 1 ? " or " : ", ") + EVAL_WIDTHS[w].name;
    }
    return fail(BP_ERR_ARG, std::string(who) + ": n_scores must be " + names);
}

int eval_cb_rate(const char *who, int fs, int n_scores)
{
    if (n_scores < BP_SCORE_ALL_N) return BP_OK;
    if (fs < 8000) return fail(BP_ERR_ARG, std::string(who) + ": sample_rate must be at least 8000 with BP_SCORE_ALL_N (the 25 bands reach 3.8 kHz)");
    if ((int)floor(0.03 * fs + 0.5) > 4096)
        return fail(BP_ERR_ARG, std::string(who) + ": sample_rate gives a frame of more than 4096 samples: too long for BP_SCORE_ALL_N (n_fft <= 8192)");
    return BP_OK;
}

namespace {

// The 25 critical bands of fwSegSNR and WSS (include/bp_c_api.h): centre frequencies and bandwidths in Hz
const double cb_cf[EV_CBN] = {50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38,
                              1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
const double cb_bw[EV_CBN] = {70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914,
                              140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};

// the supports of the 25 Gaussian filters on the bins 0 .. H - 1: first bin, bins, and the weights back to back
void cb_table(int fs, int H, std::vector<int> &band, std::vector<double> &g)
{
    band.assign((size_t)3 * EV_CBN, 0); g.clear();
    const double cut = exp(-30.0 / (2.0 * 2.303));
    for (int i = 0; i < EV_CBN; ++i) {
        const double f0 = floor(cb_cf[i] / (fs / 2.0) * H), b = cb_bw[i] / (fs / 2.0) * H;
        int lo = -1, cnt = 0;
        for (int k = 0; k < H; ++k) {
            const double u = (k - f0) / b, v = exp(-11.0 * (u * u));
            if (!(v > cut)) { if (cnt) break; continue; }            // (a Gaussian: its support is one run of bins)
            if (!cnt) lo = k;
            ++cnt; g.push_back(v);
        }
        band[i] = lo < 0 ? 0 : lo; band[EV_CBN + i] = cnt; band[2 * EV_CBN + i] = (int)g.size() - cnt;
    }
}

}  // namespace

int eval_plan(const char *who, int fs, int fea_dim, int n_scores, int n, const int *len, const int64_t *off, const int *F, EvalPlan &ep)
{
    if (!eval_rate(fs, &ep.p, &ep.q))
        return fail(BP_ERR_ARG, std::string(who) + ": sample_rate must be positive with 10000/sample_rate = p/q, max(p, q) <= 32 "
                                                   "(8, 10, 12, 16, 20, 24, 32, 48 kHz)");
    ep.n = n; ep.fs = fs; ep.D = fea_dim; ep.ns = n_scores;
    const int m = ep.p > ep.q ? ep.p : ep.q;
    ep.Lh = ep.p == 1 && ep.q == 1 ? 0 : 10 * m;                 // 10 kHz in: a copy (one tap of 1)
    ep.taps = 2 * ep.Lh + 1;
    ep.win = (int)floor(0.03 * fs + 0.5);
    ep.skip = ep.win / 4;
    { const int r = eval_cb_rate(who, fs, n_scores); if (r != BP_OK) return r; }
    ep.cH = 0; ep.cb_band.clear(); ep.cb_g.clear();
    if (ep.has(EVAL_ALL)) {                                          // n_fft = 2^ceil(log2(2 win)), H = n_fft / 2: the least power of two >= win
        for (ep.cH = 1; ep.cH < ep.win; ep.cH <<= 1) {}
        cb_table(fs, ep.cH, ep.cb_band, ep.cb_g);
    }
    ep.off.assign(off, off + n); ep.len.assign(len, len + n);
    for (std::vector<int> &v : ep.pre) v.assign((size_t)n + 1, 0);
    const int64_t LIM = INT32_MAX / 8;
    for (int s = 0; s < n; ++s) {
        const int64_t L = len[s], n10 = (L * ep.p + ep.q - 1) / ep.q;
        const int64_t J10 = n10 > EV_N ? (n10 - EV_N - 1) / EV_K + 1 : 0;   // frames j with j K < n10 - N
        const int64_t qc = (J10 * EV_K + 2 * EV_NFFT + 255) / 256 * 256;
        const int64_t pairs = J10 > EV_SEG ? (int64_t)EV_NB * (J10 - EV_SEG) : 0;
        const double jd = floor((double)L / ep.skip - (double)ep.win / ep.skip);
        const int64_t J = jd >= 1.0 ? (int64_t)jd : 0;
        int64_t nx[PRE_N];                                          // entry s + 1 of every table
        const auto at = [&ep, s](EvalPre k) { return ep.pre[k][s]; };
        nx[PRE_o10] = at(PRE_o10) + n10; nx[PRE_rb] = at(PRE_rb) + (n10 + WAVE_THREADS - 1) / WAVE_THREADS;
        nx[PRE_P] = at(PRE_P) + J10; nx[PRE_eb] = at(PRE_eb) + (J10 + 3) / 4;
        nx[PRE_Q] = at(PRE_Q) + qc; nx[PRE_qb] = at(PRE_qb) + qc / WAVE_THREADS;
        nx[PRE_CP] = at(PRE_CP) + pairs; nx[PRE_cb] = at(PRE_cb) + (pairs + WAVE_THREADS - 1) / WAVE_THREADS;
        nx[PRE_SJ] = at(PRE_SJ) + J; nx[PRE_sb] = at(PRE_sb) + (J + 3) / 4;
        nx[PRE_F] = F[s + 1]; nx[PRE_FS] = F[s + 1] + s + 1;
        for (int k = 0; k < PRE_N; ++k) {
            if (nx[k] > LIM) return fail(BP_ERR_ARG, std::string(who) + ": too many samples in one call");
            ep.pre[k][s + 1] = (int)nx[k];
        }
    }
    // resampler: h[j] = kaiser_{2Lh+1, 5}[j] sinc((j - Lh) / m), normalised to sum 1, times p (double, rounded once)
    ep.h.assign((size_t)ep.taps, 1.0f);
    if (ep.Lh > 0) {
        std::vector<double> hd((size_t)ep.taps);
        const double pi = 3.141592653589793238462643383279502884, i0b = bessel_i0(5.0);
        double sum = 0.0;
        for (int j = 0; j < ep.taps; ++j) {
            const double r = 2.0 * j / (ep.taps - 1) - 1.0, kw = bessel_i0(5.0 * sqrt(fmax(0.0, 1.0 - r * r))) / i0b;
            const double xs = (double)(j - ep.Lh) / m, sc = xs == 0.0 ? 1.0 : sin(pi * xs) / (pi * xs);
            hd[j] = kw * sc; sum += hd[j];
        }
        for (int j = 0; j < ep.taps; ++j) ep.h[j] = (float)(hd[j] / sum * ep.p);
    }
    const double pi2 = 6.283185307179586476925286766559;
    ep.v.assign(EV_NFFT, 0.0f);
    for (int i = 0; i < EV_N; ++i) ep.v[i] = (float)(0.5 * (1.0 - cos(pi2 * (i + 1) / (EV_N + 1))));
    ep.w.assign((size_t)ep.win, 0.0);
    for (int i = 0; i < ep.win; ++i) ep.w[i] = 0.5 * (1.0 - cos(pi2 * (i + 1) / (ep.win + 1)));
    ep.t_bytes = tab_layout(ep).bytes;
    return BP_OK;
}

void eval_fill(const EvalPlan &ep, char *tab)
{
    const TabLayout t = tab_layout(ep);
    memset(tab, 0, t.bytes);
    memcpy(tab + t.off, ep.off.data(), (size_t)ep.n * 8);
    memcpy(tab + t.len, ep.len.data(), (size_t)ep.n * 4);
    for (int k = 0; k < PRE_N; ++k) memcpy(tab + t.pre[k], ep.pre[k].data(), ((size_t)ep.n + 1) * 4);
    memcpy(tab + t.h, ep.h.data(), ep.h.size() * 4);
    memcpy(tab + t.v, ep.v.data(), ep.v.size() * 4);
    const double pi2 = 6.283185307179586476925286766559;
    float2 *tw = (float2 *)(tab + t.tw);
    for (int k = 0; k <= EV_NFFT / 2; ++k) tw[k] = make_float2((float)cos(pi2 * k / EV_NFFT), (float)-sin(pi2 * k / EV_NFFT));
    memcpy(tab + t.w, ep.w.data(), ep.w.size() * 8);
    if (ep.has(EVAL_ALL)) {
        double *ctw = (double *)(tab + t.ctw);
        for (int k = 0; k <= ep.cH; ++k) { ctw[2 * k] = cos(pi2 * k / (2.0 * ep.cH)); ctw[2 * k + 1] = -sin(pi2 * k / (2.0 * ep.cH)); }
        memcpy(tab + t.cband, ep.cb_band.data(), ep.cb_band.size() * 4);
        memcpy(tab + t.cg, ep.cb_g.data(), ep.cb_g.size() * 8);
    }
}

size_t eval_work_bytes(const EvalPlan &ep, int nsig) { return work_walk(ep, nsig); }

hipError_t eval_launch(const EvalPlan &ep, const EvalDev &d, int nsig, hipStream_t st)
{
    const TabLayout t = tab_layout(ep);
    EvalArgs a; memset(&a, 0, sizeof(a));
    a.off = (const int64_t *)(d.tab + t.off); a.len = (const int *)(d.tab + t.len);
#define X(name) a.name = (const int *)(d.tab + t.pre[PRE_##name]);
    EVAL_PRE(X)
#undef X
    a.h = (const float *)(d.tab + t.h); a.v = (const float *)(d.tab + t.v); a.tw = (const float2 *)(d.tab + t.tw); a.w = (const double *)(d.tab + t.w);
    a.n = ep.n; a.p = ep.p; a.q = ep.q; a.Lh = ep.Lh; a.taps = ep.taps; a.win = ep.win; a.skip = ep.skip; a.D = ep.D;
    a.clip = 1.0 + pow(10.0, 15.0 / 20.0);
    for (int k = 0; k < nsig; ++k) { a.sig[k] = d.sig[k]; a.lps[k] = d.lps[k]; }
    work_walk(ep, nsig, &a, d.work);
    a.nsig = nsig;
    a.ctw = (const double2 *)(d.tab + t.ctw); a.cband = (const int *)(d.tab + t.cband); a.cg = (const double *)(d.tab + t.cg); a.cH = ep.cH;
    a.scores = d.scores; a.ns = ep.ns;
    const int n = ep.n, ne = nsig - 1, SJ = ep.tot(PRE_SJ);
    const dim3 blk(WAVE_THREADS), per_row((unsigned)n, (unsigned)ne);
    const auto rank = [&](int nval, const double *v0, const double *v1, const int *valid, int *sel) {
        a.rank = RankSel{{v0, v1}, nval, valid, sel};
        hipLaunchKernelGGL(bp_eval_lpcrank, dim3((unsigned)((SJ + WAVE_THREADS - 1) / WAVE_THREADS), (unsigned)ne), blk, 0, st, a);
    };
    // (grids that can be empty -- no STOI or SSNR frame in the whole call -- are skipped)
    hipLaunchKernelGGL(bp_eval_resample, dim3((unsigned)ep.tot(PRE_rb), (unsigned)nsig), blk, 0, st, a);
    if (ep.tot(PRE_eb)) hipLaunchKernelGGL(bp_eval_energy, dim3((unsigned)ep.tot(PRE_eb)), blk, 0, st, a);
    hipLaunchKernelGGL(bp_eval_mask, dim3((unsigned)n), blk, 0, st, a);
    hipLaunchKernelGGL(bp_eval_compact, dim3((unsigned)ep.tot(PRE_qb), (unsigned)nsig), blk, 0, st, a);
    if (ep.tot(PRE_P))
        hipLaunchKernelGGL(bp_eval_bands, dim3((unsigned)ep.tot(PRE_P), (unsigned)nsig), blk,
                           lds_bytes(1 << EV_LOG2M) + (size_t)(EV_BIN_HI - EV_BIN_LO) * 4, st, a);
    if (ep.tot(PRE_cb)) hipLaunchKernelGGL(bp_eval_corr, dim3((unsigned)ep.tot(PRE_cb), (unsigned)ne), blk, 0, st, a);
    if (ep.tot(PRE_sb)) hipLaunchKernelGGL(bp_eval_ssnr, dim3((unsigned)ep.tot(PRE_sb), (unsigned)ne), blk, 0, st, a);
    hipLaunchKernelGGL(bp_eval_lsd, dim3((unsigned)((ep.tot(PRE_F) + 3) / 4), (unsigned)ne), blk, 0, st, a);
    if (ep.has(EVAL_EXT)) {
        if (ep.tot(PRE_CP)) hipLaunchKernelGGL(bp_eval_estoi, dim3((unsigned)(ep.tot(PRE_CP) / EV_NB)), dim3(64), 0, st, a);
        hipLaunchKernelGGL(bp_eval_sisdr, per_row, blk, 0, st, a);
    }
    hipLaunchKernelGGL(bp_eval_reduce, per_row, blk, 0, st, a);
    if (ep.has(EVAL_FULL)) {                                        // LLR and CD: order 10 below 10 kHz, else 16
        if (SJ) {
            const int P = ep.fs < 10000 ? 10 : 16;
            const size_t lds = (lpc_slab_doubles(ep.win) + (size_t)(nsig * (P + 1) + P + 1) * EV_FB) * 8;
            const dim3 fb((unsigned)((SJ + EV_FB - 1) / EV_FB));
            if (P == 10) hipLaunchKernelGGL(bp_eval_lpc<10>, fb, blk, lds, st, a);
            else hipLaunchKernelGGL(bp_eval_lpc<16>, fb, blk, lds, st, a);
            rank(2, a.llr, a.lcd, a.lv, a.lsel);
        }
        hipLaunchKernelGGL(bp_eval_lpcsum, per_row, blk, 0, st, a);
    }
    if (ep.has(EVAL_ALL)) {                                         // fwSegSNR and WSS
        if (SJ) {
            const size_t lds = cb_lds_bytes(ep.cH, nsig);
            if (lds > 65536) {
                const hipError_t e = hipFuncSetAttribute((const void *)bp_eval_cb, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) return e;
            }
            hipLaunchKernelGGL(bp_eval_cb, dim3((unsigned)((SJ + EV_CF - 1) / EV_CF)), blk, lds, st, a);
            rank(1, a.ws, nullptr, a.wv, a.csel);
        }
        hipLaunchKernelGGL(bp_eval_cbsum, per_row, blk, 0, st, a);
    }
    return hipGetLastError();
}

hipError_t eval_trim_launch(const EvalPlan &ep, const char *tab, int hop, float *pcm, hipStream_t st)
{
    const TabLayout t = tab_layout(ep);
    hipLaunchKernelGGL(bp_eval_trim, dim3((unsigned)ep.tot(PRE_FS)), dim3(WAVE_THREADS), 0, st, (const int64_t *)(tab + t.off),
                       (const int *)(tab + t.len), (const int *)(tab + t.pre[PRE_FS]), ep.n, hop, pcm);
    return hipGetLastError();
}

// bp_score_waves (n_scores = BP_SCORE_N) and bp_score_waves_ext: one sequence, the score stride apart
static int score_waves_run(const char *who, int device, int fea_dim, int sample_rate, int n_sent, const int *sent_len, const float *ref,
                           const float *est, int n_scores, float *scores)
{
    { const int r = eval_n_scores(who, n_scores); if (r != BP_OK) return r; }
    if (wave_log2_fft(fea_dim) < 0) return fail(BP_ERR_ARG, std::string(who) + ": 2*(fea_dim-1) must be a power of two from 64 to 2048");
    { int p, q; if (!eval_rate(sample_rate, &p, &q)) return fail(BP_ERR_ARG, std::string(who) + ": sample_rate must be positive with 10000/sample_rate = p/q, max(p, q) <= 32"); }
    { const int r = eval_cb_rate(who, sample_rate, n_scores); if (r != BP_OK) return r; }
    if (!est || !scores) return fail(BP_ERR_ARG, std::string(who) + ": no sentences or null pointer");
    WavePlan wp;
    { const int r = plan_waves(who, fea_dim, n_sent, sent_len, ref, (size_t)INT32_MAX / 8, wp); if (r != BP_OK) return r; }
    const int D = fea_dim;
    const size_t f = wp.frames, padded = wp.padded;
    std::vector<int64_t> off(n_sent);
    for (int s = 0; s < n_sent; ++s) off[s] = ((int64_t)wp.F[s] + s + 1) * wp.hop;   // the padded layout of bp_wave_lps
    EvalPlan ep;
    { const int r = eval_plan(who, sample_rate, D, n_scores, n_sent, sent_len, off.data(), wp.F.data(), ep); if (r != BP_OK) return r; }
    // one host->device block: tables | analysis window | twiddles | padded reference | padded estimate
    Layout lay(al256(ep.t_bytes));
    const size_t o_win = lay.take((size_t)wp.N * 4), o_tw = lay.take((size_t)(wp.M + 1) * 8), o_ref = lay.take(padded * 4);
    const size_t o_est = lay.take(padded * 4), in_b = lay.size();
    // behind it: the two LPS blocks | scores | work block
    const size_t lps_b = f * D * 4, o_lps = lay.take(lps_b), o_lps1 = lay.take(lps_b), o_sc = lay.take((size_t)n_sent * n_scores * 4);
    const size_t o_work = lay.size();
    OneShot os;
    { const int r = os.open(who, device, o_work + eval_work_bytes(ep, 2)); if (r != BP_OK) return r; }
    std::vector<char> hb(in_b, 0);
    eval_fill(ep, hb.data());
    wave_window_twiddles(wp.log2M, (float *)(hb.data() + o_win), (float2 *)(hb.data() + o_tw));
    wave_scatter((float *)(hb.data() + o_ref), wp, sent_len, ref);
    wave_scatter((float *)(hb.data() + o_est), wp, sent_len, est);
    hipError_t &e = os.e;
    char *d = os.d.as<char>();
    if (e == hipSuccess) e = hipMemcpyAsync(d, hb.data(), in_b, hipMemcpyHostToDevice, os.st);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        WaveAnaArgs a; memset(&a, 0, sizeof(a));
        a.pcm = (const float *)(d + (k ? o_est : o_ref)); a.win = (const float *)(d + o_win); a.tw = (const float2 *)(d + o_tw);
        a.F = (const int *)(d + tab_layout(ep).pre[PRE_F]);
        a.n_sent = n_sent; a.log2M = wp.log2M; a.D = D; a.hop = wp.hop; a.ctx = 1;
        a.lps = (float *)(d + (k ? o_lps1 : o_lps));
        e = wave_analysis_launch(a, (int)f, os.st);
    }
    if (e == hipSuccess) {
        EvalDev v; memset(&v, 0, sizeof(v));
        v.tab = d; v.work = d + o_work;
        v.sig[0] = (const float *)(d + o_ref); v.sig[1] = (const float *)(d + o_est);
        v.lps[0] = (const float *)(d + o_lps); v.lps[1] = (const float *)(d + o_lps1);
        v.scores = (float *)(d + o_sc);
        e = eval_launch(ep, v, 2, os.st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(scores, d + o_sc, (size_t)n_sent * n_scores * 4, hipMemcpyDeviceToHost, os.st);
    return os.finish(who);
}

extern "C" int bp_score_waves(int device, int fea_dim, int sample_rate, int n_sent, const int *sent_len, const float *ref, const float *est,
                              float *scores)
{
    return score_waves_run("bp_score_waves", device, fea_dim, sample_rate, n_sent, sent_len, ref, est, BP_SCORE_N, scores);
}

extern "C" int bp_score_waves_ext(int device, int fea_dim, int sample_rate, int n_sent, const int *sent_len, const float *ref,
                                  const float *est, int n_scores, float *scores)
{
    return score_waves_run("bp_score_waves_ext", device, fea_dim, sample_rate, n_sent, sent_len, ref, est, n_scores, scores);
}
