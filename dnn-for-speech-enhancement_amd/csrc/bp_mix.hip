// bp_mix.hip -- C-ABI implementation (include/bp_c_api.h): training mixtures made on the device.  A clean-speech
// corpus and a noise corpus stay resident on the handle (bp_set_mix_corpus); every call mixes its list of {clean, noise, offset,
// SNR} on the device, runs the analysis of bp_wave.hip on the mixtures and writes the window chunk that the training / CV step
// reads.  gfx950 only.
//
// Device layout of one call: mixture m is a "sentence" of bp_wave.hip's padded layout -- its T_m + 1 segments of hop samples start
// at segment Fs[m] = F[m] + m (F = prefix sums of T), sample i of the mixture lies at padded sample (Fs[m] + 1) hop + i, and frame
// t at (Fs[m] + t) hop.  Three such buffers: x (mixed), s (clean), g v (scaled noise).  The per-call input is ONE host->device
// copy (`MixIn`: F | Fs | clean | noise | offset | snr | order); the order table is the only per-frame data the host sends.
//
// Kernels, each a launch on the handle's stream:
//   bp_mix_gain      one workgroup per mixture: E_s and E_v in double (per-thread strided sums, then a fixed LDS tree), the gain
//   bp_mix_pcm       one workgroup per segment: x = fmaf(g, v, s), s and g v into the padded buffers (padding written as zeros)
//   bp_wave_analysis (bp_wave.hip) on x: the staged normalised rows, win_start / nat_row, the noisy LPS (bp_mix_features)
//   bp_mix_targets   one workgroup per frame: the FFTs of s and g v in LDS, one after the other, and the frame's target row
//   bp_wave_mel      (bp_wave.hip, with bp_set_mix_aux) on s: the MFCC columns of the target row, between the LPS and the mask
//   bp_wave_nat      (bp_wave.hip) the noise-aware rows; in BP_NAT_DYNAMIC (bp_set_nat) bp_wave_dnat: one row per frame from the noisy
//                    spectrum, which the calls that keep none hold behind those rows for the tracker alone
//   bp_mix_tables    per row i: win_start / targ_frame / nat_row of mixture-frame order[i]
//   bp_mix_reverb_fir  (bp_room.hip; bp_set_mix_reverb, once per call, not per mixture) clean sentences convolved with room impulse
//                    responses: the derived entries n_clean + k of the corpus; bp_mix_gain and bp_mix_pcm read
//                    an entry's mixing signal, bp_mix_pcm writes its target signal into s
// bp_eval_mix runs the same sequence without the targets, keeps the noisy spectrum Y, then bp_enhance_waves'
// forward / synthesis / overlap-add on it and the scoring kernels of bp_eval.hip (bp_eval.h) on s, x and the enhanced samples.
// bp_eval_mix_logmmse is the same call with the log-MMSE recursion of bp_classic.hip (bp_classic.h) in place of
// the forward: its gain rows go where the net's output columns went.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "bp_classic.h"
#include "bp_eval.h"
#include "bp_fft.h"
#include "bp_handle.h"
#include "bp_mel.h"
#include "bp_philox_host.h"
#include "bp_room.h"

namespace {

struct MixArgs {
    const float *clean, *noise;                                  // the corpus, back to back
    const int64_t *clean_off, *clean_len, *noise_off, *noise_len;
    const float *rev, *rev_t; const ReverbJob *rjob; int n_clean;   // derived entries n_clean + k: mixing and target signals at rjob[k].dst
    const int *Fs, *mc, *mn; const int64_t *mo; const float *msnr;  // per mixture
    int n_mix, hop;
    float *gain;                                                 // [n_mix]
    float *x, *s, *v;                                            // padded [Fs[n_mix] hop]
};

// clean entry c: its mixing signal, its target signal (the same samples for a dry entry) and its length
__device__ __forceinline__ void mix_entry(const MixArgs &a, int c, const float *&sm, const float *&st, int64_t &len)
{
    if (c < a.n_clean) { sm = st = a.clean + a.clean_off[c]; len = a.clean_len[c]; }
    else { const ReverbJob &j = a.rjob[c - a.n_clean]; sm = a.rev + j.dst; st = a.rev_t + j.dst; len = j.n; }
}

}  // namespace

__global__ __launch_bounds__(WAVE_THREADS) void bp_mix_gain(const MixArgs a)
{
    __shared__ double es[WAVE_THREADS], ev[WAVE_THREADS];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int c = a.mc[m], n = a.mn[m];
    const float *cs, *ts; int64_t lc;
    mix_entry(a, c, cs, ts, lc);
    (void)ts;                                                    // (E_s is the mixing signal's)
    const int64_t ln = a.noise_len[n], step = WAVE_THREADS % ln;
    const float *ns = a.noise + a.noise_off[n];
    double s2 = 0.0, v2 = 0.0;
    int64_t p = (a.mo[m] + tid) % ln;                            // noise sample of clean sample i = tid, tid + 256, ...
    for (int64_t i = tid; i < lc; i += WAVE_THREADS) {
        const double sv = cs[i], vv = ns[p];
        s2 += sv * sv; v2 += vv * vv;
        p += step; if (p >= ln) p -= ln;
    }
    es[tid] = s2; ev[tid] = v2;
    __syncthreads();
    for (int w = WAVE_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) { es[tid] += es[tid + w]; ev[tid] += ev[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double Es = es[0], Ev = ev[0];
        a.gain[m] = Ev > 0.0 ? (float)sqrt(Es / (Ev * pow(10.0, (double)a.msnr[m] / 10.0))) : 0.0f;
    }
}

__global__ __launch_bounds__(WAVE_THREADS) void bp_mix_pcm(const MixArgs a)
{
    const int q = blockIdx.x, m = sentence_of(a.Fs, a.n_mix, q);
    const int c = a.mc[m], n = a.mn[m];
    const float *cs, *ts; int64_t lc;                            // mixing and target signal (one pointer for a dry entry)
    mix_entry(a, c, cs, ts, lc);
    const int64_t ln = a.noise_len[n], o = a.mo[m];
    const float *ns = a.noise + a.noise_off[n];
    const float g = a.gain[m];
    const int64_t i0 = (int64_t)(q - a.Fs[m] - 1) * a.hop;     // mixture sample at the segment's first position (front pad: hop)
    for (int r = threadIdx.x; r < a.hop; r += blockDim.x) {
        const int64_t i = i0 + r;
        float xv = 0.0f, sv = 0.0f, vv = 0.0f;
        if (i >= 0 && i < lc) {
            const float s = cs[i], v = ns[(o + i) % ln];
            xv = fmaf(g, v, s); sv = ts[i]; vv = g * v;
        }
        const size_t d = (size_t)q * a.hop + r;
        a.x[d] = xv; a.s[d] = sv; a.v[d] = vv;
    }
}

namespace {
struct MixTargArgs {
    const float *s, *v; const float *win; const float2 *tw; const int *F;
    int n_mix, log2M, D, hop, target, ldt;
    float thr;                                                   // 10^(lc_db / 10)
    float *targ;                                                 // [frames][ldt]
    int col2;                                                    // first column of a two-part target's second part: D, or D + n_ceps behind the MFCC columns (bp_set_mix_aux)
};
}  // namespace

__global__ __launch_bounds__(WAVE_THREADS) void bp_mix_targets(const MixTargArgs a)
{
    extern __shared__ float2 z[];
    const int g = blockIdx.x, M = 1 << a.log2M, tid = threadIdx.x;
    float *pS = reinterpret_cast<float *>(z + lds_bytes(M) / sizeof(float2));   // |S|^2 [M + 1]: each thread reads back its own bins
    const int m = sentence_of(a.F, a.n_mix, g);
    const size_t at = (size_t)(g + m) * a.hop;
    rfft_frame(z, a.s + at, a.win, a.tw, a.log2M);
    for (int k = tid; k <= M; k += blockDim.x) { const float2 X = rfft_bin(z, a.tw, M, k); pS[k] = X.x * X.x + X.y * X.y; }
    __syncthreads();                                             // (z is reloaded below)
    rfft_frame(z, a.v + at, a.win, a.tw, a.log2M);
    float *t = a.targ + (size_t)g * a.ldt;
    for (int k = tid; k <= M; k += blockDim.x) {
        const float2 X = rfft_bin(z, a.tw, M, k);
        const float ps = pS[k], pn = X.x * X.x + X.y * X.y;
        const float lps = lps_of(ps), irm = sqrtf(ps / fmaxf(ps + pn, 1e-10f)), ibm = ps > a.thr * pn ? 1.0f : 0.0f;
        switch (a.target) {
        case BP_MIX_LPS: t[k] = lps; break;
        case BP_MIX_IRM: t[k] = irm; break;
        case BP_MIX_IBM: t[k] = ibm; break;
        case BP_MIX_LPS_IRM: t[k] = lps; t[a.col2 + k] = irm; break;
        default: t[k] = lps; t[a.col2 + k] = ibm; break;
        }
    }
}

// row i of the chunk trains mixture-frame g = order[i] (identity without order): its window starts at staged row g + m (ctx - 1)
__global__ __launch_bounds__(WAVE_THREADS) void bp_mix_tables(const int *__restrict__ order, const int *__restrict__ F, int n_mix, int n,
                                                           int ctx, int *__restrict__ ws, int *__restrict__ tf, int *__restrict__ nr, int nat_frame)
{
    const int i = blockIdx.x * WAVE_THREADS + threadIdx.x;
    if (i >= n) return;
    const int g = order ? order[i] : i, m = sentence_of(F, n_mix, g);
    ws[i] = g + m * (ctx - 1);
    tf[i] = g;
    if (nr) nr[i] = nat_frame ? g : m;                           // the noise-aware row of the mixture, or (BP_NAT_DYNAMIC) of the frame itself
}

// ------------------------------------------------------------------ host side
struct MixState {
    int D, log2M, M, hop, ctx, toff, target, sL;
    bool nat;
    float thr;
    bool aux; MelDev mel;                                        // bp_set_mix_aux when the corpus was set: the MFCC columns [D, D + mel.n_ceps) and their tables (h->aux_tab)
    int n_clean, n_noise, n_pair;                                // n_pair: derived entries n_clean .. n_clean + n_pair - 1
    std::vector<int64_t> clean_len, noise_len;                   // clean_len: [n_clean + n_pair]
    Buf reverb;                                                  // device: r | e (early target only) | ReverbJob [n_pair]
    size_t o_rv_t, o_rv_job;
    Buf corpus;                                                  // device: clean | noise | offsets and lengths | mean | inv_std | window | twiddles
    size_t o_clean, o_noise, o_cl_off, o_cl_len, o_no_off, o_no_len, o_mean, o_istd, o_win, o_tw;
    Buf in_d, x, s, v, gain, lps;                                // grow-only device buffers of the calls
    Buf in_pin[2]; Event ev_in[2]; bool ev_valid[2]; int pin_cur;   // pinned input blocks, alternating
    Buf ev_Y, ev_syn, ev_ola, ev_lps, ev_tab, ev_work, ev_pin;   // bp_eval_mix (ev_pin: pinned table block)
    Buf ev_gain;                                                 // bp_eval_mix_logmmse: gain rows [frames][D] | vad [frames]
};

namespace {


int parts_of(int target) { return target == BP_MIX_LPS_IRM || target == BP_MIX_LPS_IBM ? 2 : 1; }

// The frame plan of a call, checked before any device work.
struct Call {
    int n;
    std::vector<int> F, Fs;                                      // [n + 1]
    size_t frames, rows, segs;                                   // frames, staged rows, padded segments
    size_t o_F, o_Fs, o_c, o_n, o_o, o_snr, o_order, bytes;      // MixIn layout
};
int plan_call(const bp_handle *h, const char *who, int n_mix, const bp_mixture *m, Call &c)
{
    if (!h) return fail(BP_ERR_ARG, std::string(who) + ": null handle");
    const MixState *ms = h->mix;
    if (!ms) return fail(BP_ERR_STATE, std::string(who) + ": no corpus (bp_set_mix_corpus)");
    if (h->dp) return fail(BP_ERR_STATE, std::string(who) + ": not on an attached data-parallel handle");
    if (n_mix < 1 || !m) return fail(BP_ERR_ARG, std::string(who) + ": no mixtures or null pointer");
    c.n = n_mix;
    c.F.assign((size_t)n_mix + 1, 0); c.Fs.assign((size_t)n_mix + 1, 0);
    size_t f = 0;
    for (int i = 0; i < n_mix; ++i) {
        const bp_mixture &x = m[i];
        if (x.clean < 0 || x.clean >= ms->n_clean + ms->n_pair) return fail(BP_ERR_ARG, std::string(who) + ": mixture " + std::to_string(i) + ": clean index out of range");
        if (x.noise < 0 || x.noise >= ms->n_noise) return fail(BP_ERR_ARG, std::string(who) + ": mixture " + std::to_string(i) + ": noise index out of range");
        if (x.offset < 0 || x.offset >= ms->noise_len[x.noise])
            return fail(BP_ERR_ARG, std::string(who) + ": mixture " + std::to_string(i) + ": offset outside the noise recording");
        if (!std::isfinite(x.snr_db)) return fail(BP_ERR_ARG, std::string(who) + ": mixture " + std::to_string(i) + ": SNR is not finite");
        f += (size_t)((ms->clean_len[x.clean] - 1) / ms->hop + 2);
        if (f > (size_t)h->cap) break;                            // (caught below; keeps the sums small)
        c.F[i + 1] = (int)f; c.Fs[i + 1] = (int)f + i + 1;
    }
    c.frames = f;
    c.rows = f + (size_t)n_mix * (ms->ctx - 1);
    if (c.rows > (size_t)h->cap)
        return fail(BP_ERR_ARG, std::string(who) + ": frames + n_mix*(context-1) exceed the chunk capacity " + std::to_string(h->cap));
    c.segs = (size_t)c.Fs[n_mix];
    Layout lay;
    c.o_F = lay.take(((size_t)n_mix + 1) * 4); c.o_Fs = lay.take(((size_t)n_mix + 1) * 4);
    c.o_c = lay.take((size_t)n_mix * 4); c.o_n = lay.take((size_t)n_mix * 4); c.o_o = lay.take((size_t)n_mix * 8);
    c.o_snr = lay.take((size_t)n_mix * 4); c.o_order = lay.take(c.frames * 4); c.bytes = lay.size();
    return BP_OK;
}

int check_order(const char *who, const Call &c, const int *order)
{
    if (!order) return BP_OK;
    std::vector<char> seen(c.frames, 0);
    for (size_t i = 0; i < c.frames; ++i) {
        const int g = order[i];
        if (g < 0 || (size_t)g >= c.frames || seen[g]) return fail(BP_ERR_ARG, std::string(who) + ": order is not a permutation of [0, frames)");
        seen[g] = 1;
    }
    return BP_OK;
}

// Mix, analyse and write the window chunk of a call into the staging set that is not current (targets included unless !targets),
// on h->stream.  Then the caller adopts it.  lps_out: also keep the noisy LPS in ms->lps; Y: also keep the noisy spectrum there.
int generate(bp_handle *h, const Call &c, const bp_mixture *m, const int *order, bool lps_out, float **rows_out, float **targ_out,
             float **nat_out, float2 *Y = nullptr, bool targets = true)
{
    MixState *ms = h->mix;
    HIPCHK(hipSetDevice(h->cfg.device));
    const int D = ms->D, n = (int)c.frames;
    const size_t pcm_b = c.segs * ms->hop * 4;
    int r = wave_grow(h, {{ms->in_d, c.bytes, false}, {ms->x, pcm_b, false}, {ms->s, pcm_b, false}, {ms->v, pcm_b, false},
                          {ms->gain, (size_t)c.n * 4, false}, {ms->lps, lps_out ? c.frames * D * 4 : 0, false}});
    if (r != BP_OK) return r;
    float *rows_d, *targ_d, *nat_d; int *tab;
    targ_d = nullptr;
    // BP_NAT_DYNAMIC (bp_set_nat; the callers have checked that the net has the block): one noise-aware row per frame from the
    // noisy spectrum, which a call that keeps none (Y == null) holds behind the rows, in the same buffer, for the tracker alone
    const bool dyn = ms->nat && h->nat_mode == BP_NAT_DYNAMIC;
    const size_t dnat_b = al256(c.frames * D * 4);
    const size_t nat_b = !ms->nat ? 0 : !dyn ? (size_t)c.n * D * 4 : Y ? c.frames * D * 4 : dnat_b + c.frames * D * sizeof(float2);
    if ((r = window_reserve(h, c.rows * D * 4, targets ? c.frames * ms->sL * 4 : 0, nat_b, c.frames, &rows_d,
                            targets ? &targ_d : nullptr, &nat_d, &tab)) != BP_OK)
        return r;
    if (dyn && !Y) Y = (float2 *)((char *)nat_d + dnat_b);
    // the pinned input block: the copy out of this one was enqueued two calls ago; wait for it (not for the training behind it)
    const int k = ms->pin_cur;
    ms->pin_cur ^= 1;
    if (ms->ev_valid[k]) HIPCHK(hipEventSynchronize(ms->ev_in[k]));
    if ((r = wave_grow(h, {{ms->in_pin[k], c.bytes, true}})) != BP_OK) return r;
    char *hb = (char *)ms->in_pin[k].p, *db = (char *)ms->in_d.p;
    memcpy(hb + c.o_F, c.F.data(), c.F.size() * 4);
    memcpy(hb + c.o_Fs, c.Fs.data(), c.Fs.size() * 4);
    for (int i = 0; i < c.n; ++i) {
        ((int *)(hb + c.o_c))[i] = m[i].clean; ((int *)(hb + c.o_n))[i] = m[i].noise;
        ((int64_t *)(hb + c.o_o))[i] = m[i].offset; ((float *)(hb + c.o_snr))[i] = m[i].snr_db;
    }
    const size_t in_b = order ? c.bytes : c.o_order;
    if (order) memcpy(hb + c.o_order, order, c.frames * 4);
    HIPCHK(hipMemcpyAsync(db, hb, in_b, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(ms->ev_in[k], h->stream));
    ms->ev_valid[k] = true;

    const char *cp = ms->corpus.as<char>();
    const float *win = (const float *)(cp + ms->o_win);
    const float2 *tw = (const float2 *)(cp + ms->o_tw);
    const int *F = (const int *)(db + c.o_F);
    MixArgs a; memset(&a, 0, sizeof(a));
    a.clean = (const float *)(cp + ms->o_clean); a.noise = (const float *)(cp + ms->o_noise);
    a.clean_off = (const int64_t *)(cp + ms->o_cl_off); a.clean_len = (const int64_t *)(cp + ms->o_cl_len);
    a.noise_off = (const int64_t *)(cp + ms->o_no_off); a.noise_len = (const int64_t *)(cp + ms->o_no_len);
    a.n_clean = ms->n_clean;
    if (ms->n_pair) {
        const char *rv = ms->reverb.as<char>();
        a.rev = (const float *)rv; a.rev_t = (const float *)(rv + ms->o_rv_t);
        a.rjob = (const ReverbJob *)(rv + ms->o_rv_job);
    }
    a.Fs = (const int *)(db + c.o_Fs); a.mc = (const int *)(db + c.o_c); a.mn = (const int *)(db + c.o_n);
    a.mo = (const int64_t *)(db + c.o_o); a.msnr = (const float *)(db + c.o_snr);
    a.n_mix = c.n; a.hop = ms->hop; a.gain = (float *)ms->gain.p;
    a.x = (float *)ms->x.p; a.s = (float *)ms->s.p; a.v = (float *)ms->v.p;
    hipLaunchKernelGGL(bp_mix_gain, dim3((unsigned)c.n), dim3(WAVE_THREADS), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(bp_mix_pcm, dim3((unsigned)c.segs), dim3(WAVE_THREADS), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    {
        WaveAnaArgs w; memset(&w, 0, sizeof(w));
        w.pcm = a.x; w.win = win; w.tw = tw; w.F = F;
        w.mean = (const float *)(cp + ms->o_mean); w.inv_std = (const float *)(cp + ms->o_istd);
        w.n_sent = c.n; w.log2M = ms->log2M; w.D = D; w.hop = ms->hop; w.ctx = ms->ctx; w.toff = ms->toff;
        w.lps = lps_out ? (float *)ms->lps.p : nullptr; w.rows = rows_d; w.Y = Y;
        w.win_start = tab; w.nat_row = ms->nat ? tab + 2 * (size_t)n : nullptr; w.nat_frame = dyn;
        HIPCHK(wave_analysis_launch(w, n, h->stream));
    }
    if (targets) {
        MixTargArgs t; memset(&t, 0, sizeof(t));
        t.s = a.s; t.v = a.v; t.win = win; t.tw = tw; t.F = F;
        t.n_mix = c.n; t.log2M = ms->log2M; t.D = D; t.hop = ms->hop; t.target = ms->target; t.ldt = ms->sL; t.thr = ms->thr;
        t.col2 = ms->aux ? D + ms->mel.n_ceps : D;
        t.targ = targ_d;
        hipLaunchKernelGGL(bp_mix_targets, dim3((unsigned)n), dim3(WAVE_THREADS), lds_bytes(ms->M) + (size_t)(ms->M + 1) * 4, h->stream, t);
        HIPCHK(hipGetLastError());
        if (ms->aux) {
            MelArgs q; memset(&q, 0, sizeof(q));
            q.pcm = a.s; q.win = win; q.tw = tw; q.F = F;
            q.n_sent = c.n; q.log2M = ms->log2M; q.D = D; q.hop = ms->hop; q.m = ms->mel;
            q.mfcc = targ_d; q.ldm = ms->sL; q.col = D;
            HIPCHK(wave_mel_launch(q, n, h->stream));
        }
    }
    if (dyn)
        HIPCHK(wave_dnat_launch(h->nat_np, Y, F, c.n, D, (const float *)(cp + ms->o_mean), (const float *)(cp + ms->o_istd), nat_d, h->stream));
    else if (ms->nat) HIPCHK(wave_nat_launch(rows_d, F, c.n, D, ms->ctx, ms->toff, nat_d, h->stream));
    hipLaunchKernelGGL(bp_mix_tables, dim3((unsigned)((n + WAVE_THREADS - 1) / WAVE_THREADS)), dim3(WAVE_THREADS), 0, h->stream,
                       order ? (const int *)(db + c.o_order) : (const int *)nullptr, F, c.n, n, ms->ctx, tab, tab + n,
                       ms->nat ? tab + 2 * (size_t)n : (int *)nullptr, (int)dyn);
    HIPCHK(hipGetLastError());
    if (rows_out) *rows_out = rows_d;
    if (targ_out) *targ_out = targ_d;
    if (nat_out) *nat_out = nat_d;
    return BP_OK;
}

}  // namespace

void mix_free(bp_handle *h)
{
    if (h->mix)
        for (Event &e : h->mix->ev_in) if (e) (void)hipEventSynchronize(e);   // (the copy out of a pinned input block may still run)
    delete h->mix;
    h->mix = nullptr;
}

extern "C" int bp_set_mix_corpus(bp_handle *h, const bp_mix_corpus *c)
{
    if (!h || !c) return fail(BP_ERR_ARG, "bp_set_mix_corpus: null handle or corpus");
    if (h->dp) return fail(BP_ERR_STATE, "bp_set_mix_corpus: not on an attached data-parallel handle");
    const int log2M = wave_log2_fft(c->fea_dim);
    if (log2M < 0) return fail(BP_ERR_ARG, "bp_set_mix_corpus: 2*(fea_dim-1) must be a power of two from 64 to 2048");
    const int D = c->fea_dim, ctx = c->context, toff = c->targ_offset, L = h->L, sL = h->s[L - 1];
    if (ctx < 1 || toff < 0 || toff >= ctx) return fail(BP_ERR_ARG, "bp_set_mix_corpus: need context >= 1 and 0 <= targ_offset < context");
    const bool nat = (long)h->s[0] == (long)(ctx + 1) * D;
    if (!nat && (long)h->s[0] != (long)ctx * D)
        return fail(BP_ERR_ARG, "bp_set_mix_corpus: layersizes[0] must be context*fea_dim or (context+1)*fea_dim");
    if (c->target < BP_MIX_LPS || c->target > BP_MIX_LPS_IBM) return fail(BP_ERR_ARG, "bp_set_mix_corpus: unknown target");
    MelTab mel;
    if (h->aux_on) {                                             // bp_set_mix_aux: [LPS | MFCC | mask]
        if (c->target != BP_MIX_LPS && c->target != BP_MIX_LPS_IRM && c->target != BP_MIX_LPS_IBM)
            return fail(BP_ERR_ARG, "bp_set_mix_corpus: with the MFCC auxiliary target (bp_set_mix_aux) the target must begin with LPS (LPS, LPS+IRM, LPS+IBM)");
        const long want = (long)parts_of(c->target) * D + h->aux.n_ceps;
        if ((long)sL != want)
            return fail(BP_ERR_ARG, "bp_set_mix_corpus: layersizes[last] must be parts*fea_dim + n_ceps = " + std::to_string(want) +
                                        " with the MFCC auxiliary target (bp_set_mix_aux)");
        const int r = mel_tables("bp_set_mix_corpus", D, h->aux, mel);
        if (r != BP_OK) return r;
    } else if ((long)sL != (long)parts_of(c->target) * D) {
        return fail(BP_ERR_ARG, "bp_set_mix_corpus: layersizes[last] must be fea_dim (LPS, IRM, IBM) or 2*fea_dim (LPS+IRM, LPS+IBM)");
    }
    if (!std::isfinite(c->lc_db)) return fail(BP_ERR_ARG, "bp_set_mix_corpus: lc_db is not finite");
    if (!c->mean || !c->inv_std) return fail(BP_ERR_ARG, "bp_set_mix_corpus: null mean / inv_std");
    if (c->n_clean < 1 || c->n_noise < 1 || !c->clean_len || !c->noise_len || !c->clean_pcm || !c->noise_pcm)
        return fail(BP_ERR_ARG, "bp_set_mix_corpus: need at least one clean sentence and one noise recording");
    size_t nc = 0, nn = 0;
    for (int i = 0; i < c->n_clean; ++i) {
        if (c->clean_len[i] < 1) return fail(BP_ERR_ARG, "bp_set_mix_corpus: empty clean sentence " + std::to_string(i));
        if ((c->clean_len[i] - 1) / ((int64_t)1 << log2M) + 2 > (int64_t)h->cap)
            return fail(BP_ERR_ARG, "bp_set_mix_corpus: clean sentence " + std::to_string(i) + " is longer than one chunk");
        nc += (size_t)c->clean_len[i];
    }
    for (int i = 0; i < c->n_noise; ++i) {
        if (c->noise_len[i] < 1) return fail(BP_ERR_ARG, "bp_set_mix_corpus: empty noise recording " + std::to_string(i));
        nn += (size_t)c->noise_len[i];
    }
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipStreamSynchronize(h->stream));                     // (an earlier corpus may still be read)
    mix_free(h);
    MixState *ms = new MixState();
    ms->D = D; ms->log2M = log2M; ms->M = 1 << log2M; ms->hop = ms->M; ms->ctx = ctx; ms->toff = toff; ms->target = c->target; ms->sL = sL;
    ms->nat = nat; ms->thr = (float)pow(10.0, (double)c->lc_db / 10.0);
    ms->n_clean = c->n_clean; ms->n_noise = c->n_noise;
    ms->clean_len.assign(c->clean_len, c->clean_len + c->n_clean);
    ms->noise_len.assign(c->noise_len, c->noise_len + c->n_noise);
    Layout lay;
    ms->o_clean = lay.take(nc * 4); ms->o_noise = lay.take(nn * 4);
    ms->o_cl_off = lay.take((size_t)c->n_clean * 8); ms->o_cl_len = lay.take((size_t)c->n_clean * 8);
    ms->o_no_off = lay.take((size_t)c->n_noise * 8); ms->o_no_len = lay.take((size_t)c->n_noise * 8);
    ms->o_mean = lay.take((size_t)D * 4); ms->o_istd = lay.take((size_t)D * 4);
    ms->o_win = lay.take((size_t)2 * ms->M * 4); ms->o_tw = lay.take((size_t)(ms->M + 1) * 8);
    const size_t bytes = lay.size();
    h->mix = ms;
    if (ms->corpus.alloc(bytes) != hipSuccess) { mix_free(h); return fail(BP_ERR_NOMEM, "bp_set_mix_corpus: hipMalloc (corpus)"); }
    for (int k = 0; k < 2; ++k)
        if (ms->ev_in[k].create(hipEventDisableTiming) != hipSuccess) { mix_free(h); return fail(BP_ERR_DEVICE, "bp_set_mix_corpus: event"); }
    std::vector<char> small(bytes - ms->o_cl_off);
    char *sb = small.data() - ms->o_cl_off;                      // (indexed with the block's offsets)
    std::vector<int64_t> off(c->n_clean, 0);
    for (int i = 1; i < c->n_clean; ++i) off[i] = off[i - 1] + c->clean_len[i - 1];
    memcpy(sb + ms->o_cl_off, off.data(), off.size() * 8);
    memcpy(sb + ms->o_cl_len, c->clean_len, (size_t)c->n_clean * 8);
    off.assign(c->n_noise, 0);
    for (int i = 1; i < c->n_noise; ++i) off[i] = off[i - 1] + c->noise_len[i - 1];
    memcpy(sb + ms->o_no_off, off.data(), off.size() * 8);
    memcpy(sb + ms->o_no_len, c->noise_len, (size_t)c->n_noise * 8);
    memcpy(sb + ms->o_mean, c->mean, (size_t)D * 4);
    memcpy(sb + ms->o_istd, c->inv_std, (size_t)D * 4);
    wave_window_twiddles(log2M, (float *)(sb + ms->o_win), (float2 *)(sb + ms->o_tw));
    char *cp = ms->corpus.as<char>();
    hipError_t e = hipMemcpy(cp + ms->o_clean, c->clean_pcm, nc * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(cp + ms->o_noise, c->noise_pcm, nn * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(cp + ms->o_cl_off, small.data(), small.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && h->aux_on) {                          // the tables of this fea_dim into the handle's block (nothing reads it: the stream is idle)
        const MelBlock mb = mel_block(mel.n_mel, mel.n_ceps, mel_packed_weights(mel));
        std::vector<char> tb(mb.bytes, 0);
        mel_block_fill(tb.data(), mb, h->aux, mel);
        e = hipMemcpy(h->aux_tab, tb.data(), mb.bytes, hipMemcpyHostToDevice);
        ms->aux = true; ms->mel = mel_dev((const char *)h->aux_tab, mb, mel);
    }
    if (e != hipSuccess) { mix_free(h); return fail(BP_ERR_DEVICE, std::string("bp_set_mix_corpus: ") + hipGetErrorString(e)); }
    return BP_OK;
}

// The MFCC auxiliary target of the next bp_set_mix_corpus (include/bp_c_api.h).  Every check before anything is
// touched; the table block is allocated by the first call that turns the target on, at the parameter limits, and never again.
extern "C" int bp_set_mix_aux(bp_handle *h, const bp_mel_params *p)
{
    if (!h) return fail(BP_ERR_ARG, "bp_set_mix_aux: null handle");
    if (h->dp) return fail(BP_ERR_STATE, "bp_set_mix_aux: not on an attached data-parallel handle");
    if (!p) { h->aux_on = false; return BP_OK; }
    MelP m;
    { const int r = mel_check("bp_set_mix_aux", p, m); if (r != BP_OK) return r; }
    if (!h->aux_tab) {
        HIPCHK(hipSetDevice(h->cfg.device));
        const int r = dev_alloc(h, &h->aux_tab, mel_block_limit() / 4);
        if (r != BP_OK) return r;
    }
    h->aux = m; h->aux_on = true;
    return BP_OK;
}

extern "C" int bp_train_mix(bp_handle *h, int n_mix, const bp_mixture *m, const int *order)
{
    Call c;
    int r;
    if ((r = plan_call(h, "bp_train_mix", n_mix, m, c)) != BP_OK || (r = check_order("bp_train_mix", c, order)) != BP_OK) return r;
    if (h->Bg != h->B) return fail(BP_ERR_STATE, "bp_train_mix: data-parallel handle (global_bunchsize != bunchsize)");
    bool dyn;
    if ((r = wave_nat_mode("bp_train_mix", h, h->mix->nat, &dyn)) != BP_OK) return r;
    if ((r = generate(h, c, m, order, false, nullptr, nullptr, nullptr)) != BP_OK) return r;
    if ((r = window_adopt(h, (int)c.frames, h->mix->D, h->mix->ctx, h->mix->nat, true)) != BP_OK) return r;
    return train_whole_chunk(h, (int)c.frames);
}

extern "C" int bp_cv_mix(bp_handle *h, int n_mix, const bp_mixture *m, float *sum)
{
    Call c;
    int r;
    if ((r = plan_call(h, "bp_cv_mix", n_mix, m, c)) != BP_OK) return r;
    if (!sum) return fail(BP_ERR_ARG, "bp_cv_mix: null argument");
    bool dyn;
    if ((r = wave_nat_mode("bp_cv_mix", h, h->mix->nat, &dyn)) != BP_OK) return r;
    const int n = (int)c.frames, L = h->L, sL = h->s[L - 1];
    if ((r = out_chunk_reserve(h, n)) != BP_OK) return r;
    float *targ_d;
    if ((r = generate(h, c, m, nullptr, false, nullptr, &targ_d, nullptr)) != BP_OK) return r;
    // forward without staging the targets (as bp_cv_chunk_windows); the target frames stay in the set for the sum below
    if ((r = window_adopt(h, n, h->mix->D, h->mix->ctx, h->mix->nat, false)) != BP_OK) return r;
    if ((r = forward_resident_as(h, n, BP_FORWARD_DEFAULT)) != BP_OK) return r;      // (CV: the step's kernels in either mode)
    std::vector<float> tg((size_t)n * sL);
    if ((r = outputs_to_host(h, n)) != BP_OK) return r;
    HIPCHK(hipMemcpyAsync(tg.data(), targ_d, tg.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *sum = sq_err_sum(h->host_out.as<float>(), h->ld[L - 1], sL, n, [&](int j) { return tg.data() + (size_t)j * sL; });
    return BP_OK;
}

extern "C" int bp_mix_features(bp_handle *h, int n_mix, const bp_mixture *m, float *fea, float *lps, float *targ, float *nat, float *pcm)
{
    Call c;
    int r;
    if ((r = plan_call(h, "bp_mix_features", n_mix, m, c)) != BP_OK) return r;
    MixState *ms = h->mix;
    if (nat && !ms->nat) return fail(BP_ERR_ARG, "bp_mix_features: nat requested for a net without the noise-aware block");
    bool dyn;
    if ((r = wave_nat_mode("bp_mix_features", h, ms->nat, &dyn)) != BP_OK) return r;
    const int D = ms->D, n = (int)c.frames;
    float *rows_d, *targ_d, *nat_d;
    if ((r = generate(h, c, m, nullptr, lps != nullptr, &rows_d, &targ_d, &nat_d)) != BP_OK) return r;
    if ((r = window_adopt(h, n, D, ms->ctx, ms->nat, true)) != BP_OK) return r;
    std::vector<float> rows(fea ? c.rows * D : 0), x(pcm ? c.segs * ms->hop : 0);
    if (fea) HIPCHK(hipMemcpyAsync(rows.data(), rows_d, rows.size() * 4, hipMemcpyDeviceToHost, h->stream));
    if (lps) HIPCHK(hipMemcpyAsync(lps, ms->lps.p, c.frames * D * 4, hipMemcpyDeviceToHost, h->stream));
    if (targ) HIPCHK(hipMemcpyAsync(targ, targ_d, c.frames * ms->sL * 4, hipMemcpyDeviceToHost, h->stream));
    if (nat) HIPCHK(hipMemcpyAsync(nat, nat_d, (dyn ? c.frames : (size_t)c.n) * D * 4, hipMemcpyDeviceToHost, h->stream));
    if (pcm) HIPCHK(hipMemcpyAsync(x.data(), ms->x.p, x.size() * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    size_t dst = 0;
    for (int i = 0; i < c.n; ++i) {
        const int T = c.F[i + 1] - c.F[i];
        if (fea)
            memcpy(fea + (size_t)c.F[i] * D, rows.data() + ((size_t)c.F[i] + (size_t)i * (ms->ctx - 1) + ms->toff) * D, (size_t)T * D * 4);
        if (pcm) {
            const int64_t len = ms->clean_len[m[i].clean];
            memcpy(pcm + dst, x.data() + ((size_t)c.Fs[i] + 1) * ms->hop, (size_t)len * 4);
            dst += (size_t)len;
        }
    }
    return BP_OK;
}

// bp_eval_mix (lm == null: the net's output columns [out_col, out_col + D) as `target`) and bp_eval_mix_logmmse (lm: the checked
// parameters; the gain rows of the recursion as BP_WAVE_MASK): one sequence, one enhancer swapped for the other.  bp_gv_mix (gv:
// where its sums go) is the same generate -> adopt -> forward with the net; then, in place of resynthesis and scoring, the LPS of
// the clean signal and the sums over the net's columns (gv->post: over their post-processed values).
struct GvOut { bool post; double *sums[4]; };
static int eval_mix_run(const char *who, bp_handle *h, const LogmmseP *lm, const NoiseP &nz, const Call &c, const bp_mixture *m, int sample_rate, int target,
                        int out_col, int NS, float *noisy_scores, float *enh_scores, float *enh_pcm, const GvOut *gv = nullptr)
{
    int r;
    const int n_mix = c.n;
    MixState *ms = h->mix;
    const int D = ms->D, L = h->L, n = (int)c.frames, hop = ms->hop;
    if (!gv && (!noisy_scores || !enh_scores)) return fail(BP_ERR_ARG, std::string(who) + ": null scores");
    std::vector<int> len(n_mix);
    std::vector<int64_t> off(n_mix);
    for (int i = 0; i < n_mix; ++i) { len[i] = (int)ms->clean_len[m[i].clean]; off[i] = ((int64_t)c.Fs[i] + 1) * hop; }
    EvalPlan ep;
    if (!gv && (r = eval_plan(who, sample_rate, D, NS, n_mix, len.data(), off.data(), c.F.data(), ep)) != BP_OK) return r;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (gv && !h->gv_parts && (r = dev_alloc(h, &h->gv_parts, (size_t)(GV_PARTS + 1) * 4 * POST_MAX_D * 2)) != BP_OK) return r;
    // every buffer first (a growth waits for the stream), then the sequence without a host wait (gv: Y and the clean LPS alone)
    const size_t pcm_b = gv ? 0 : c.segs * hop * 4, lps_b = al256(c.frames * D * 4), sc_b = gv ? 0 : (size_t)2 * n_mix * NS * 4;
    const size_t tab_b = gv ? 0 : ep.t_bytes;
    r = wave_grow(h, {{ms->ev_Y, c.frames * D * sizeof(float2), false}, {ms->ev_syn, gv ? 0 : c.frames * 2 * hop * 4, false}, {ms->ev_ola, pcm_b, false},
                      {ms->ev_lps, gv ? lps_b : 2 * lps_b, false}, {ms->ev_tab, tab_b + sc_b, false}, {ms->ev_work, gv ? 0 : eval_work_bytes(ep, 3), false},
                      {ms->ev_pin, tab_b, true}, {ms->lps, gv ? 0 : c.frames * D * 4, false},
                      {ms->ev_gain, lm ? c.frames * ((size_t)D + 1) * 4 : 0, false}});
    if (r != BP_OK) return r;
    if (!lm && (r = out_chunk_reserve(h, n)) != BP_OK) return r;
    // the table block: the pinned buffer is free (the previous call ended in a synchronisation)
    char *tab = (char *)ms->ev_tab.p;
    if (!gv) {
        eval_fill(ep, (char *)ms->ev_pin.p);
        HIPCHK(hipMemcpyAsync(tab, ms->ev_pin.p, ep.t_bytes, hipMemcpyHostToDevice, h->stream));
    }
    float2 *Y = (float2 *)ms->ev_Y.p;
    if ((r = generate(h, c, m, nullptr, !gv, nullptr, nullptr, nullptr, Y, false)) != BP_OK) return r;
    if ((r = window_adopt(h, n, D, ms->ctx, ms->nat, false)) != BP_OK) return r;
    if (!lm && (r = forward_resident(h, n)) != BP_OK) return r;
    const char *cp = ms->corpus.as<char>();
    const float *win = (const float *)(cp + ms->o_win);
    const float2 *tw = (const float2 *)(cp + ms->o_tw);
    const int *F = (const int *)((const char *)ms->in_d.p + c.o_F);
    float *ola = (float *)ms->ev_ola.p, *lps_s = (float *)ms->ev_lps.p, *lps_e = (float *)((char *)ms->ev_lps.p + lps_b);
    if (gv) {
        WaveAnaArgs w; memset(&w, 0, sizeof(w));                   // the LPS of s, as the scoring below analyses it for LSD
        w.pcm = (const float *)ms->s.p; w.win = win; w.tw = tw; w.F = F;
        w.n_sent = n_mix; w.log2M = ms->log2M; w.D = D; w.hop = hop; w.ctx = 1; w.lps = lps_s;
        HIPCHK(wave_analysis_launch(w, n, h->stream));
        HIPCHK(wave_gv_launch(h, h->out_chunk.as<float>(), h->ld[L - 1], out_col, Y, lps_s, D, n, gv->post ? &h->post : nullptr, h->stream));
        const double *tot = reinterpret_cast<const double *>(h->gv_parts) + (size_t)GV_PARTS * 4 * D;
        for (int k = 0; k < 4; ++k)
            HIPCHK(hipMemcpyAsync(gv->sums[k], tot + (size_t)k * D, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return BP_OK;
    }
    if (lm) {
        float *gain = (float *)ms->ev_gain.p;
        HIPCHK(logmmse_gain_launch(*lm, nz, Y, F, n_mix, D, gain, gain + c.frames * D, nullptr, h->stream));
        HIPCHK(wave_synthesis_launch(gain, D, 0, Y, win, tw, ms->log2M, D, BP_WAVE_MASK, (float *)ms->ev_syn.p, n, h->stream));
    } else
        HIPCHK(wave_synthesis_launch(h->out_chunk.as<float>(), h->ld[L - 1], out_col, Y, win, tw, ms->log2M, D, target, (float *)ms->ev_syn.p, n, h->stream,
                                     h->post_on ? &h->post : nullptr));
    HIPCHK(wave_overlap_launch((const float *)ms->ev_syn.p, win, F, n_mix, hop, ola, n, h->stream));
    HIPCHK(eval_trim_launch(ep, tab, hop, ola, h->stream));        // = the enhanced sentences in bp_score_waves' padded layout
    for (int k = 0; k < 2; ++k) {                                  // the LPS of s and of the enhanced samples (x's: generate)
        WaveAnaArgs w; memset(&w, 0, sizeof(w));
        w.pcm = k ? ola : (const float *)ms->s.p; w.win = win; w.tw = tw; w.F = F;
        w.n_sent = n_mix; w.log2M = ms->log2M; w.D = D; w.hop = hop; w.ctx = 1;
        w.lps = k ? lps_e : lps_s;
        HIPCHK(wave_analysis_launch(w, n, h->stream));
    }
    {
        EvalDev d; memset(&d, 0, sizeof(d));
        d.tab = tab; d.work = (char *)ms->ev_work.p;
        d.sig[0] = (const float *)ms->s.p; d.sig[1] = (const float *)ms->x.p; d.sig[2] = ola;
        d.lps[0] = lps_s; d.lps[1] = (const float *)ms->lps.p; d.lps[2] = lps_e;
        d.scores = (float *)(tab + al256(ep.t_bytes));
        HIPCHK(eval_launch(ep, d, 3, h->stream));
    }
    std::vector<float> sc((size_t)2 * n_mix * NS), pcm(enh_pcm ? c.segs * hop : 0);
    HIPCHK(hipMemcpyAsync(sc.data(), tab + al256(ep.t_bytes), sc_b, hipMemcpyDeviceToHost, h->stream));
    if (enh_pcm) HIPCHK(hipMemcpyAsync(pcm.data(), ola, pcm_b, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(noisy_scores, sc.data(), (size_t)n_mix * NS * 4);
    memcpy(enh_scores, sc.data() + (size_t)n_mix * NS, (size_t)n_mix * NS * 4);
    if (enh_pcm) {
        size_t dst = 0;
        for (int i = 0; i < n_mix; ++i) { memcpy(enh_pcm + dst, pcm.data() + off[i], (size_t)len[i] * 4); dst += (size_t)len[i]; }
    }
    return BP_OK;
}

// bp_eval_mix (n_scores = BP_SCORE_N) and bp_eval_mix_ext
static int eval_mix_net(const char *who, bp_handle *h, int n_mix, const bp_mixture *m, int sample_rate, int target, int out_col, int n_scores,
                        float *noisy_scores, float *enh_scores, float *enh_pcm)
{
    Call c;
    int r;
    if ((r = eval_n_scores(who, n_scores)) != BP_OK || (r = plan_call(h, who, n_mix, m, c)) != BP_OK) return r;
    const int D = h->mix->D, sL = h->s[h->L - 1];
    if (target != BP_WAVE_LPS && target != BP_WAVE_MASK) return fail(BP_ERR_ARG, std::string(who) + ": target must be BP_WAVE_LPS or BP_WAVE_MASK");
    if (out_col < 0 || (long)out_col + D > sL) return fail(BP_ERR_ARG, std::string(who) + ": out_col + fea_dim exceeds layersizes[last]");
    bool dyn;
    if ((r = wave_nat_mode(who, h, h->mix->nat, &dyn)) != BP_OK || (r = wave_post_check(who, h, D, target)) != BP_OK) return r;
    return eval_mix_run(who, h, nullptr, noise_vad(), c, m, sample_rate, target, out_col, n_scores, noisy_scores, enh_scores, enh_pcm);
}

// The second moments of the GV factors over the mixtures of a plan (include/bp_c_api.h): a mode of eval_mix_run
extern "C" int bp_gv_mix(bp_handle *h, int n_mix, const bp_mixture *m, int out_col, int stage, double *est_sum, double *est_sq, double *ref_sum,
                         double *ref_sq, int64_t *frames)
{
    Call c;
    int r;
    if ((r = plan_call(h, "bp_gv_mix", n_mix, m, c)) != BP_OK) return r;
    const int D = h->mix->D, sL = h->s[h->L - 1];
    if (stage != BP_GV_RAW && stage != BP_GV_POST) return fail(BP_ERR_ARG, "bp_gv_mix: stage must be BP_GV_RAW or BP_GV_POST");
    if (out_col < 0 || (long)out_col + D > sL) return fail(BP_ERR_ARG, "bp_gv_mix: out_col + fea_dim exceeds layersizes[last]");
    if (!est_sum || !est_sq || !ref_sum || !ref_sq || !frames) return fail(BP_ERR_ARG, "bp_gv_mix: null output");
    bool dyn;
    if ((r = wave_nat_mode("bp_gv_mix", h, h->mix->nat, &dyn)) != BP_OK) return r;
    const GvOut gv = {stage == BP_GV_POST && h->post_on, {est_sum, est_sq, ref_sum, ref_sq}};
    if (gv.post && (r = wave_post_check("bp_gv_mix", h, D, BP_WAVE_LPS)) != BP_OK) return r;
    if ((r = eval_mix_run("bp_gv_mix", h, nullptr, noise_vad(), c, m, 0, BP_WAVE_LPS, out_col, 0, nullptr, nullptr, nullptr, &gv)) != BP_OK) return r;
    *frames = (int64_t)c.frames;
    return BP_OK;
}

// bp_eval_mix_logmmse (n_scores = BP_SCORE_N), bp_eval_mix_logmmse_ext and (nt: the noise update of np; else the VAD-gated one
// whatever np) bp_eval_mix_logmmse_nt
static int eval_mix_lm(const char *who, bp_handle *h, const bp_logmmse_params *p, bool nt, const bp_noise_params *np, int n_mix, const bp_mixture *m, int sample_rate, int n_scores,
                       float *noisy_scores, float *enh_scores, float *enh_pcm)
{
    Call c;
    LogmmseP lp;
    NoiseP nz = noise_vad();
    int r;
    if ((r = eval_n_scores(who, n_scores)) != BP_OK || (r = logmmse_check(who, p, lp)) != BP_OK || (nt && (r = noise_check(who, np, nz)) != BP_OK) ||
        (r = plan_call(h, who, n_mix, m, c)) != BP_OK) return r;
    return eval_mix_run(who, h, &lp, nz, c, m, sample_rate, BP_WAVE_MASK, 0, n_scores, noisy_scores, enh_scores, enh_pcm);
}

extern "C" int bp_eval_mix(bp_handle *h, int n_mix, const bp_mixture *m, int sample_rate, int target, int out_col, float *noisy_scores,
                           float *enh_scores, float *enh_pcm)
{
    return eval_mix_net("bp_eval_mix", h, n_mix, m, sample_rate, target, out_col, BP_SCORE_N, noisy_scores, enh_scores, enh_pcm);
}

extern "C" int bp_eval_mix_ext(bp_handle *h, int n_mix, const bp_mixture *m, int sample_rate, int target, int out_col, int n_scores,
                               float *noisy_scores, float *enh_scores, float *enh_pcm)
{
    return eval_mix_net("bp_eval_mix_ext", h, n_mix, m, sample_rate, target, out_col, n_scores, noisy_scores, enh_scores, enh_pcm);
}

extern "C" int bp_eval_mix_logmmse(bp_handle *h, const bp_logmmse_params *p, int n_mix, const bp_mixture *m, int sample_rate,
                                   float *noisy_scores, float *enh_scores, float *enh_pcm)
{
    return eval_mix_lm("bp_eval_mix_logmmse", h, p, false, nullptr, n_mix, m, sample_rate, BP_SCORE_N, noisy_scores, enh_scores, enh_pcm);
}

extern "C" int bp_eval_mix_logmmse_ext(bp_handle *h, const bp_logmmse_params *p, int n_mix, const bp_mixture *m, int sample_rate, int n_scores,
                                       float *noisy_scores, float *enh_scores, float *enh_pcm)
{
    return eval_mix_lm("bp_eval_mix_logmmse_ext", h, p, false, nullptr, n_mix, m, sample_rate, n_scores, noisy_scores, enh_scores, enh_pcm);
}

extern "C" int bp_eval_mix_logmmse_nt(bp_handle *h, const bp_logmmse_params *p, const bp_noise_params *np, int n_mix, const bp_mixture *m,
                                      int sample_rate, int n_scores, float *noisy_scores, float *enh_scores, float *enh_pcm)
{
    return eval_mix_lm("bp_eval_mix_logmmse_nt", h, p, true, np, n_mix, m, sample_rate, n_scores, noisy_scores, enh_scores, enh_pcm);
}

extern "C" int bp_mix_plan(uint64_t seed, int n_clean, int per_clean, int n_noise, const int64_t *noise_len, int n_snr,
                           const float *snr_db, bp_mixture *out)
{
    if (n_clean < 1 || per_clean < 1 || n_noise < 1 || n_snr < 1 || !noise_len || !snr_db || !out)
        return fail(BP_ERR_ARG, "bp_mix_plan: need n_clean, per_clean, n_noise, n_snr >= 1 and non-null arrays");
    if ((int64_t)n_clean * per_clean > INT32_MAX) return fail(BP_ERR_ARG, "bp_mix_plan: too many mixtures");
    for (int k = 0; k < n_noise; ++k)
        if (noise_len[k] < 1 || noise_len[k] >= ((int64_t)1 << 32)) return fail(BP_ERR_ARG, "bp_mix_plan: noise_len must lie in [1, 2^32)");
    for (int k = 0; k < n_snr; ++k)
        if (!std::isfinite(snr_db[k])) return fail(BP_ERR_ARG, "bp_mix_plan: SNR is not finite");
    const int n = n_clean * per_clean;
    for (int m = 0; m < n; ++m) {
        uint32_t c[4] = {(uint32_t)m, 0, 0, 0};
        philox(c, seed);
        bp_mixture &x = out[m];
        memset(&x, 0, sizeof(x));
        x.clean = m / per_clean;
        x.noise = (int)scale(c[0], (uint64_t)n_noise);
        x.offset = (int64_t)scale(c[1], (uint64_t)noise_len[x.noise]);
        x.snr_db = snr_db[scale(c[2], (uint64_t)n_snr)];
    }
    for (int i = n - 1; i > 0; --i) {
        const int j = (int)scale(word0(seed, (uint32_t)i, 0, 1), (uint64_t)i + 1);
        const bp_mixture t = out[i]; out[i] = out[j]; out[j] = t;
    }
    return BP_OK;
}

extern "C" int bp_mix_shuffle(uint64_t seed, uint32_t stream, int n, int *order)
{
    if (n < 0 || (n > 0 && !order)) return fail(BP_ERR_ARG, "bp_mix_shuffle: bad n or null order");
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = n - 1; i > 0; --i) {
        const int j = (int)scale(word0(seed, (uint32_t)i, stream, 2), (uint64_t)i + 1);
        const int t = order[i]; order[i] = order[j]; order[j] = t;
    }
    return BP_OK;
}

// The reverberant entries of the corpus: the checks, the job list and the kernel are bp_room.hip's (bp_room.h)
extern "C" int bp_set_mix_reverb(bp_handle *h, const bp_mix_reverb *r)
{
    if (!h || !r) return fail(BP_ERR_ARG, "bp_set_mix_reverb: null handle or argument");
    std::vector<int64_t> off;
    std::vector<int> delay;
    int rc;
    if ((rc = check_rirs("bp_set_mix_reverb", r->n_rir, r->rir_len, r->rir_pcm, r->early_taps, off, delay)) != BP_OK) return rc;
    if (r->n_pair < 1 || !r->pair_clean || !r->pair_rir) return fail(BP_ERR_ARG, "bp_set_mix_reverb: need at least one pair and non-null pair arrays");
    if (r->target != BP_REVERB_TARGET_REVERBERANT && r->target != BP_REVERB_TARGET_EARLY)
        return fail(BP_ERR_ARG, "bp_set_mix_reverb: unknown target");
    for (int k = 0; k < r->n_pair; ++k)
        if (r->pair_rir[k] < 0 || r->pair_rir[k] >= r->n_rir)
            return fail(BP_ERR_ARG, "bp_set_mix_reverb: pair " + std::to_string(k) + ": response index out of range");
    MixState *ms = h->mix;
    if (!ms) return fail(BP_ERR_STATE, "bp_set_mix_reverb: no corpus (bp_set_mix_corpus)");
    if (h->dp) return fail(BP_ERR_STATE, "bp_set_mix_reverb: not on an attached data-parallel handle");
    std::vector<int64_t> coff((size_t)ms->n_clean + 1, 0);
    for (int i = 0; i < ms->n_clean; ++i) coff[i + 1] = coff[i] + ms->clean_len[i];
    std::vector<ReverbJob> job(r->n_pair);
    int64_t tot = 0;
    for (int k = 0; k < r->n_pair; ++k) {
        const int c = r->pair_clean[k];
        if (c < 0 || c >= ms->n_clean) return fail(BP_ERR_ARG, "bp_set_mix_reverb: pair " + std::to_string(k) + ": clean index out of range");
        if (ms->clean_len[c] > RV_MAX_LEN) return fail(BP_ERR_ARG, "bp_set_mix_reverb: pair " + std::to_string(k) + ": clean sentence too long");
        job[k].src = coff[c]; job[k].n = (int)ms->clean_len[c]; job[k].rir = r->pair_rir[k];
        tot += job[k].n;
    }
    const bool early = r->target == BP_REVERB_TARGET_EARLY;
    const int64_t blocks = fill_jobs(job, off, delay, r->rir_len, r->early_taps);
    if (blocks > INT32_MAX) return fail(BP_ERR_ARG, "bp_set_mix_reverb: too many samples for one call");
    Layout lay;                                                  // r | e (early target only) | jobs
    lay.take((size_t)tot * 4);
    const size_t o_t = early ? lay.take((size_t)tot * 4) : 0, o_job = lay.take(job.size() * sizeof(ReverbJob));
    const size_t bytes = lay.size(), rir_b = (size_t)off[r->n_rir] * 4;
    HIPCHK(hipSetDevice(h->cfg.device));
    Buf nb, hb;                                                  // the new entries; the responses (for this call only)
    if (nb.alloc(bytes) != hipSuccess || hb.alloc(rir_b) != hipSuccess) {
        (void)hipGetLastError();
        return fail(BP_ERR_NOMEM, "bp_set_mix_reverb: hipMalloc (the previous entries stay)");
    }
    char *nd = nb.as<char>(), *hd = hb.as<char>();
    hipError_t e = hipMemcpyAsync(nd + o_job, job.data(), job.size() * sizeof(ReverbJob), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hd, r->rir_pcm, rir_b, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        ReverbArgs a; memset(&a, 0, sizeof(a));
        a.job = (const ReverbJob *)(nd + o_job); a.n_job = r->n_pair;
        a.src = (const float *)(ms->corpus.as<char>() + ms->o_clean); a.rir = (const float *)hd;
        a.out_r = (float *)nd; a.out_e = early ? (float *)(nd + o_t) : nullptr;
        e = reverb_launch(a, blocks, early, h->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(h->stream);       // (the host arrays are the caller's; earlier calls may read the old entries)
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(BP_ERR_DEVICE, std::string("bp_set_mix_reverb: ") + hipGetErrorString(e));
    ms->reverb = std::move(nb);                                  // (the previous entries go)
    ms->o_rv_t = o_t; ms->o_rv_job = o_job; ms->n_pair = r->n_pair;
    ms->clean_len.resize(ms->n_clean);
    for (const ReverbJob &j : job) ms->clean_len.push_back(j.n);
    return BP_OK;
}
