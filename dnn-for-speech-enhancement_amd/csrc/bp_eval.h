// bp_eval.h -- the scoring launchers of bp_eval.hip, for bp_score_waves (bp_eval.hip) and bp_eval_mix (bp_mix.hip): the objective
// scores of estimates against a reference, as many columns per score row as the call asks for -- EVAL_WIDTHS below says which
// widths there are and what each adds (definitions: include/bp_c_api.h).
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

// The widths of a score row, narrowest first.  A width has the columns, work arrays, tables and kernels of every narrower one
// (whose columns keep their bits) and adds its own behind them; `adds` is the one description of that.
enum EvalWidth { EVAL_BASIC, EVAL_EXT, EVAL_FULL, EVAL_ALL, EVAL_WIDTH_N };
struct EvalWidthRow { int ns; const char *name, *adds; };
constexpr EvalWidthRow EVAL_WIDTHS[EVAL_WIDTH_N] = {
    {BP_SCORE_N, "BP_SCORE_N", "SSNR, LSD, STOI: bp_eval_resample .. bp_eval_lsd and bp_eval_reduce, which writes the row"},
    {BP_SCORE_EXT_N, "BP_SCORE_EXT_N", "ESTOI, SI-SDR: bp_eval_estoi and bp_eval_sisdr before bp_eval_reduce"},
    {BP_SCORE_FULL_N, "BP_SCORE_FULL_N", "LLR, CD: bp_eval_lpc, bp_eval_lpcrank, bp_eval_lpcsum; per-frame values in the work block"},
    {BP_SCORE_ALL_N, "BP_SCORE_ALL_N", "fwSegSNR, WSS: bp_eval_cb, bp_eval_lpcrank (on the WSS values), bp_eval_cbsum; three tables, per-frame values"},
};

// The per-sentence prefix tables ([n + 1] ints each), named once, in table-block order: X(name) makes the ids PRE_name, the
// kernels' pointers a.name and their binding.
//   o10, rb: 10 kHz samples, resampler workgroups; P, eb: STOI frames J10 (bound of C and S), energy workgroups; Q, qb: compacted
//   samples, workgroups; CP, cb: correlation pairs 15 (J10 - 30)+, workgroups; SJ, sb: SSNR frames, workgroups; F, FS: analysis
//   frames (1d), padded segments F[s] + s
#define EVAL_PRE(X) X(o10) X(rb) X(P) X(eb) X(Q) X(qb) X(CP) X(cb) X(SJ) X(sb) X(F) X(FS)
#define X(name) PRE_##name,
enum EvalPre { EVAL_PRE(X) PRE_N };
#undef X

// Host plan of one call: the per-sentence tables and where they lie in the table block.
struct EvalPlan {
    int n, fs, p, q, Lh, taps, win, skip, D;      // rate p/q = 10000/fs in lowest terms; SSNR frame / skip; fea_dim
    int ns;                                       // score columns per row: the ns of one row of EVAL_WIDTHS
    std::vector<int64_t> off;                     // [n] first sample of each sentence
    std::vector<int> len;                         // [n]
    std::vector<int> pre[PRE_N];                  // the prefix tables, by id
    int tot(EvalPre k) const { return pre[k][n]; }            // a table's last entry: its count over the whole call
    bool has(EvalWidth w) const { return ns >= EVAL_WIDTHS[w].ns; }
    std::vector<float> h, v;                      // resampler taps [taps]; STOI window [512] (second half zero)
    std::vector<double> w;                        // SSNR window [win]
    int cH;                                       // EVAL_ALL: n_fft / 2 of fwSegSNR / WSS (else 0, and the two tables empty)
    std::vector<int> cb_band;                     // [3][25] first bin, bins, offset into cb_g of the 25 band filters' supports
    std::vector<double> cb_g;                     // their weights
    size_t t_bytes;                               // table block
};
// The rate rule: 10000/fs = p/q in lowest terms, max(p, q) <= 32.
bool eval_rate(int fs, int *p, int *q);
// BP_OK for the ns of a row of EVAL_WIDTHS, else BP_ERR_ARG: the first check of every _ext call.
int eval_n_scores(const char *who, int n_scores);
// With BP_SCORE_ALL_N: BP_ERR_ARG unless fs >= 8000 (all 25 bands below Nyquist) and win <= 4096 (n_fft <= 8192).  eval_plan checks it.
int eval_cb_rate(const char *who, int fs, int n_scores);
// Checks the rate and sizes (BP_ERR_ARG, nothing touched) and builds the plan; F: [n + 1] analysis frame prefix of the call;
// n_scores: the caller has checked it with eval_n_scores.
int eval_plan(const char *who, int fs, int fea_dim, int n_scores, int n, const int *len, const int64_t *off, const int *F, EvalPlan &ep);
void eval_fill(const EvalPlan &ep, char *tab);    // the table block, t_bytes
size_t eval_work_bytes(const EvalPlan &ep, int nsig);

struct EvalDev {
    const char *tab; char *work;                  // device: the filled table block, eval_work_bytes(nsig) bytes
    const float *sig[EVAL_MAXSIG], *lps[EVAL_MAXSIG];
    float *scores;                                // [nsig - 1][n][ns]
};
// The whole scoring sequence on st: the reference side once, the estimates' sides, the per-sentence reductions, then the
// kernels of each wider row of EVAL_WIDTHS that the plan has, which write their own columns alone.
hipError_t eval_launch(const EvalPlan &ep, const EvalDev &d, int nsig, hipStream_t st);
// Zero every sample of the padded layout outside [off[s], off[s] + len[s]) of its sentence (hop-sample segments).
hipError_t eval_trim_launch(const EvalPlan &ep, const char *tab, int hop, float *pcm, hipStream_t st);
