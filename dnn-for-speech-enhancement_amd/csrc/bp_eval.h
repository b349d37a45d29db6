// bp_eval.h -- the scoring launchers of bp_eval.hip, for bp_score_waves (bp_eval.hip) and bp_eval_mix (bp_mix.hip): segmental SNR,
// log-spectral distortion and STOI of estimates against a reference, with ESTOI and SI-SDR beside them where the call asks for five
// score columns, and LLR and cepstral distance behind those with seven (definitions: include/bp_c_api.h).
// Internal: nothing in here is part of the C ABI.
//
// One call scores n sentences of nsig signals: signal 0 is the reference, signals 1 .. nsig-1 the estimates.  Sample i of sentence
// s lies at sig[k][off[s] + i] (i < len[s]) in every signal; the LSD reads the analysis (bp_wave_analysis with lps set) of every
// signal, frame t of sentence s at lps[k][(F[s] + t) D].  Everything whose size depends on the data (kept STOI frames C, STFT
// frames S = C - 1) is sized by its bound (all frames kept): the host never waits in the middle of a call.
#pragma once
#include <stdint.h>
#include <vector>

#include "bp_fft.h"

constexpr int EVAL_MAXSIG = 3;

// Host plan of one call: the per-sentence tables (prefix sums [n + 1] unless noted) and where they lie in the table block.
struct EvalPlan {
    int n, fs, p, q, Lh, taps, win, skip, D;      // rate p/q = 10000/fs in lowest terms; SSNR frame / skip; fea_dim
    int ns;                                       // score columns per row: BP_SCORE_N, BP_SCORE_EXT_N (ESTOI and SI-SDR are computed),
                                                  // BP_SCORE_FULL_N (LLR and CD as well: per-frame values in the work block) or
                                                  // BP_SCORE_ALL_N (fwSegSNR and WSS as well: their tables and per-frame values)
    std::vector<int64_t> off;                     // [n] first sample of each sentence
    std::vector<int> len;                         // [n]
    std::vector<int> o10, rb;                     // 10 kHz samples; resampler workgroups
    std::vector<int> P, eb, Q, qb;                // STOI frames J10 (bound of C and S); energy workgroups; compacted samples, workgroups
    std::vector<int> CP, cb;                      // correlation pairs 15 (J10 - 30)+; workgroups
    std::vector<int> SJ, sb;                      // SSNR frames; workgroups
    std::vector<int> F, FS;                       // analysis frames (1d); padded segments F[s] + s
    std::vector<float> h, v;                      // resampler taps [taps]; STOI window [512] (second half zero)
    std::vector<double> w;                        // SSNR window [win]
    int cH;                                       // nine columns: n_fft / 2 of fwSegSNR / WSS (else 0, and the two tables empty)
    std::vector<int> cb_band;                     // [3][25] first bin, bins, offset into cb_g of the 25 band filters' supports
    std::vector<double> cb_g;                     // their weights
    size_t t_bytes;                               // table block
};
// The rate rule: 10000/fs = p/q in lowest terms, max(p, q) <= 32.
bool eval_rate(int fs, int *p, int *q);
// BP_OK for BP_SCORE_N, BP_SCORE_EXT_N, BP_SCORE_FULL_N and BP_SCORE_ALL_N, else BP_ERR_ARG: the first check of every _ext call.
int eval_n_scores(const char *who, int n_scores);
// With BP_SCORE_ALL_N: BP_ERR_ARG unless fs >= 8000 (all 25 bands below Nyquist) and win <= 4096 (n_fft <= 8192).  eval_plan checks it.
int eval_cb_rate(const char *who, int fs, int n_scores);
// Checks the rate and sizes (BP_ERR_ARG, nothing touched) and builds the plan; F: [n + 1] analysis frame prefix of the call;
// n_scores: BP_SCORE_N, BP_SCORE_EXT_N, BP_SCORE_FULL_N or BP_SCORE_ALL_N (the caller has checked it).
int eval_plan(const char *who, int fs, int fea_dim, int n_scores, int n, const int *len, const int64_t *off, const int *F, EvalPlan &ep);
void eval_fill(const EvalPlan &ep, char *tab);    // the table block, t_bytes
size_t eval_work_bytes(const EvalPlan &ep, int nsig);

struct EvalDev {
    const char *tab; char *work;                  // device: the filled table block, eval_work_bytes(nsig) bytes
    const float *sig[EVAL_MAXSIG], *lps[EVAL_MAXSIG];
    float *scores;                                // [nsig - 1][n][ns]
};
// The whole scoring sequence on st: the reference side once, the estimates' sides, the per-sentence reductions.  With five
// columns bp_eval_estoi and bp_eval_sisdr run before the reductions; with three nothing else changes.  With seven the LLR / CD
// kernels (bp_eval_lpc, bp_eval_lpcrank, bp_eval_lpcsum) run behind the five-column sequence and write columns 5 and 6 alone; with
// nine bp_eval_cb, bp_eval_lpcrank (on the WSS values) and bp_eval_cbsum run behind those and write columns 7 and 8 alone.
hipError_t eval_launch(const EvalPlan &ep, const EvalDev &d, int nsig, hipStream_t st);
// Zero every sample of the padded layout outside [off[s], off[s] + len[s]) of its sentence (hop-sample segments).
hipError_t eval_trim_launch(const EvalPlan &ep, const char *tab, int hop, float *pcm, hipStream_t st);
