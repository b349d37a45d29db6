/*
 * bp_c_api.h -- C ABI of the MI355X-native trainer that replaces the reference's `BP_GPU`
 * object (the frame-wise DNN forward / backward / momentum-update hot path).
 *
 * Every entry point below is what a binding for this path binds.  Each cites the reference
 * interface it replaces (paths relative to the reference tree).  Plain pointers and sizes
 * only; no HIP, torch or C++ types.  All functions return 0 on success and a negative
 * bp_status on failure (the reference instead prints and calls exit(0): BP_GPU.cu:20-24,
 * 929-933 -- the C++ shim include/BP_GPU.h reproduces that convention on top of this ABI).
 * bp_last_error() returns the message of the last failure on the calling thread.
 *
 * Host data layout (identical to the reference):
 *   weights[l][p*cur + c]  (l = 1..numlayers-1, index 0 unused, [prev][cur] row-major)
 *   bias[l][c], in[f*s0 + k], targ[f*sL + d], all fp32 little-endian.
 * Ownership: the library copies in/out; it never keeps or frees caller pointers.  On return
 * from bp_train_chunk / bp_cv_chunk the caller may overwrite `in`/`targ` at once (the
 * reference gives the same guarantee through pageable-memory cublasSetVectorAsync,
 * BP_GPU.cu:274-276); bp_get_weights returns with the data in place (the reference relies
 * on pageable-memory semantics at BP_GPU.cu:920-921).
 */
#ifndef BP_C_API_H
#define BP_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BP_MAXLAYER 10          /* BP_GPU.h:13  (#define MAXLAYER 10)           */
#define BP_MAXCACHEFRAME 200000 /* BP_GPU.h:14  (#define MAXCACHEFRAME 200000)  */

typedef enum {
    BP_OK = 0,
    BP_ERR_ARG = -1,     /* bad argument / configuration                         */
    BP_ERR_DEVICE = -2,  /* HIP runtime error (message has the HIP error string) */
    BP_ERR_STATE = -3,   /* call not valid in the handle's current state         */
    BP_ERR_NOMEM = -4
} bp_status;

/* Constructor arguments of BP_GPU (BP_GPU.h:43-44, BP_GPU.cu:10-12) plus the switches the
 * reference exposes only by editing source.  A zero-initialised tail reproduces the live
 * reference behaviour. */
typedef struct bp_config {
    int   gpu_used;                 /* a_GPU_selected. Reference: device count; here the ranks of
                                       a data-parallel job are separate processes, so this is
                                       informational and must be >= 1                          */
    int   numlayers;                /* number of layer SIZES (2..9, WorkPara limit Interface.h:44) */
    int   layersizes[BP_MAXLAYER];
    int   bunchsize;                /* frames per minibatch handled by THIS device             */
    float lrate, momentum, weightcost;
    int   dropoutflag;              /* 1 = dropout on (BP_GPU.cu:534-551)                      */
    float visible_omit, hid_omit;
    /* ---- extensions (0 = live reference) ---- */
    int   activation;               /* 0 ReLU (DevFunc.cu:67-97 live) | 1 Sigmoid (.bak)        */
    int   momentum_rule;            /* 0 (1-m) rule DevFunc.cu:313-318 | 1 classic :306-311     */
    uint64_t seed;                  /* dropout Philox key (reference: time(NULL), BP_GPU.cu:77) */
    int   device;                   /* HIP device ordinal for this handle                       */
    int   global_bunchsize;         /* data parallel: frames per minibatch over ALL ranks
                                       (0 = bunchsize).  Scales dEdX_L by 2/global and the
                                       update by 1/global                        */
    int   rank_frame_offset;        /* data parallel: index of this rank's first frame inside
                                       the global bunch (keys the dropout stream)               */
    int   max_chunk_frames;         /* capacity of the resident chunk cache; 0 = BP_MAXCACHEFRAME */
    int   compute_dtype;            /* 0 = fp32 everywhere (the reference).  1 = bf16 GEMM operands
                                       (activations, errors, a shadow copy of the weights) with fp32
                                       accumulation, fp32 master weights / momentum / update
                                       (BASELINE.json configs[4]); parity tolerance 2e-2 instead of
                                       1e-4.  Every call works in this mode except
                                       bp_time_kernel (fp32 kernels only)                        */
} bp_config;

typedef struct bp_handle bp_handle;

const char *bp_last_error(void);
/* Library/ABI version and the gfx target the kernels were compiled for ("gfx950"). */
int         bp_abi_version(void);
const char *bp_build_target(void);
/* Number of MI355X devices visible to the process (hipGetDeviceCount), for hosts that do not link the HIP runtime. */
int         bp_device_count(int *n);

/* BP_GPU::BP_GPU (BP_GPU.cu:10-197): select device, allocate device state, upload weights
 * and biases (index 1..numlayers-1).  Momentum state starts at zero (devnew_vf zero-fill,
 * BP_GPU.cu:137-138,938-940). */
int bp_create(const bp_config *cfg, const float *const *weights, const float *const *bias,
              bp_handle **out);

/* BP_GPU::~BP_GPU (BP_GPU.cu:199-239). */
int bp_destroy(bp_handle *h);

/* The reference reads its public members lrate / momentum / weightcost / dropoutflag / visible_omit /
 * hid_omit afresh on every bunch (train_bunch_single: `cur_lrate = lrate`, BP_GPU.cu:488-500), so a caller
 * may change them between chunks.  This pushes new values into the handle; the C++ shim calls it at the
 * start of train() and CrossValid() with the current member values. */
int bp_set_hyper(bp_handle *h, float lrate, float momentum, float weightcost, int dropoutflag,
                 float visible_omit, float hid_omit);

/* Output-layer nonlinearity and loss (no counterpart in the live reference; its older revision BP_GPU.cu.bak:565-630
 * applies kernSigmoid to the output layer and feeds the post-sigmoid output into kernSubClean).
 * activation 0 = linear (default, = the live reference; linear_cols and loss must be 0).
 * activation 1 = logistic y = 1/(1+expf(-z)) on output columns [linear_cols, sL); columns [0, linear_cols) stay linear
 *   (z = alpha*acc + b, alpha = the CV keep-scale as for the linear output).
 * loss (logistic columns only): 0 = dEdz = (2/Bg)(y - t)            (gradient of 2*BCE/Bg w.r.t. z; targets are NOT
 *                                                                      range-checked: outside [0, 1] is the caller's business)
 *                               1 = dEdz = (2/Bg)(y - t) * y * (1 - y)  (squared error through the logistic)
 * Linear columns keep dEdz = (2/Bg)(o - t); Bg = global bunch.  Applies from the next call on, in fp32 and bf16 mode, on
 * stacked and window chunks, in bp_train_*, bp_grads_resident, bp_cv_chunk[_windows] (squared error of the post-activation
 * outputs) and bp_forward[_windows] (post-activation outputs).  On an attached data-parallel handle every rank must pass the
 * same values (as for bp_set_hyper).  Bad values (activation or loss not 0/1, linear_cols outside [0, sL) with activation 1,
 * non-zero linear_cols or loss with activation 0, null handle) return BP_ERR_ARG and leave the handle unchanged. */
int bp_set_output(bp_handle *h, int activation, int linear_cols, int loss);

/* The kernels of the INFERENCE forward: bp_forward[_windows], bp_enhance_waves, bp_eval_mix (and the forward of the mixing calls
 * that score the net) and the pushes of streams opened afterwards.  bp_train_*, bp_cv_*, bp_grads_resident, bp_profile_step and
 * bp_eval_mix_logmmse are the same in either mode.
 * BP_FORWARD_DEFAULT (0, the default): the step's forward GEMMs, today's bits.  There a frame's output can differ in the last
 *   bit with the row of the bunch it sits in.
 * BP_FORWARD_ROWINV (1): one thin-M kernel per layer (bp_infer.hip) whose summation order is fixed by the layer's shape alone.  A
 *   frame's output row is a function of the bits of its stacked input row, the weights and biases, dropoutflag and the omit
 *   rates, the hidden activation and the bp_set_output setting -- and of nothing else: not of the row's index in the chunk, the
 *   number of rows of the call, the handle's bunchsize or max_chunk_frames, what other rows hold, or the entry point.  The same
 *   bits on every run (no float atomics).  Against the default mode only the summation order differs (the same activation and
 *   output arithmetic).  On thousands of frames it runs bunch by bunch and is slower than the default.
 * A stream keeps the mode its handle had at bp_stream_open: one opened in ROWINV packs the frames of a push densely, in channel
 * order, so that a push of n frames costs ceil(n / bunchsize) bunches however many channels there are, and returns the bits of
 * bp_enhance_waves in ROWINV mode.  A later bp_set_forward does not change open streams.
 * fp32 handles (compute_dtype = 0): ROWINV on a bf16 handle returns BP_ERR_ARG.  A bad mode or a null handle returns BP_ERR_ARG;
 * the handle is unchanged after an error. */
enum { BP_FORWARD_DEFAULT = 0, BP_FORWARD_ROWINV = 1 };
int bp_set_forward(bp_handle *h, int mode);

/* BP_GPU::train (BP_GPU.cu:241-331): upload a chunk of n_frames stacked input frames and
 * targets, then run one SGD-momentum step (train_bunch_single, BP_GPU.cu:484-673) per
 * consecutive full bunch; the partial last bunch is ignored (:315-318).  Synchronous with
 * respect to `in`/`targ`. */
int bp_train_chunk(bp_handle *h, int n_frames, const float *in, const float *targ);

/* BP_GPU::CrossValid (BP_GPU.cu:408-479) + cv_bunch_single (:676-773): inference forward
 * (weights scaled by keep when dropoutflag==1), partial bunch processed, returns the SUM of
 * squared errors accumulated in fp32 in frame-major / bin-minor order (:458-467). */
int bp_cv_chunk(bp_handle *h, int n_frames, const float *in, const float *targ,
                float *sq_err_sum);

/* cv_bunch_single (BP_GPU.cu:676-773) exposed for parity tests and batch enhancement:
 * out[n_frames][sL] = network(in) with CV semantics. */
int bp_forward(bp_handle *h, int n_frames, const float *in, float *out);

/* BP_GPU::returnWeights (BP_GPU.cu:910-923). */
int bp_get_weights(bp_handle *h, float *const *weights, float *const *bias);
/* Momentum state (delta_weights/delta_bias, BP_WorkSpace BP_GPU.h:35-36); the reference never
 * downloads it -- provided for parity tests and checkpointing. */
int bp_get_deltas(bp_handle *h, float *const *delta_weights, float *const *delta_bias);

/* ------------------------------------------------------------------------------------
 * Resident-chunk interface: the same step as bp_train_chunk, split so that a caller who
 * already has the chunk in device memory (benchmarks, on-device data producers) can drive
 * bunches without the host upload.  bp_upload_chunk = the H2D part of BP_GPU::train
 * (BP_GPU.cu:269-277); bp_train_resident = the bunch loop (:294-326) over frames
 * [first_frame, first_frame + n_frames) of the resident chunk.  Asynchronous: returns after
 * enqueueing; bp_sync waits. */
int bp_upload_chunk(bp_handle *h, int n_frames, const float *in, const float *targ);
int bp_fill_chunk_synthetic(bp_handle *h, int n_frames, uint64_t seed); /* N(0,1) in/targ on device */
int bp_train_resident(bp_handle *h, int first_frame, int n_frames);
int bp_sync(bp_handle *h);
/* Parity-test entry: bp_train_resident with CALLER-SUPPLIED dropout masks instead of the Philox stream (the reference's
 * masks come from cuRAND seeded by time(NULL), BP_GPU.cu:77-78,534-551, so "same result given the same mask" is the
 * parity statement).  masks[l], l = 0 .. numlayers-2: host [n_frames][layersizes[l]] bytes, 1 = drop the output of
 * layer l for that frame (l = 0: the input frame); NULL = no dropout on that layer.  fp32 single-device handles. */
int bp_train_resident_masked(bp_handle *h, int first_frame, int n_frames, const uint8_t *const *masks);
/* What is resident, and what may train on it.  Every call that takes data makes its chunk the handle's resident chunk, the
 * queries too: bp_forward and bp_cv_chunk (stacked), bp_forward_windows, bp_cv_chunk_windows, bp_enhance_waves, the mixing calls
 * and a stream's push (window).  bp_train_resident[_masked], bp_grads_resident and bp_profile_step work on whatever is resident:
 * A frame range outside the resident chunk returns BP_ERR_ARG (checked first).
 * A chunk whose targets were not supplied by the call that made it resident returns BP_ERR_STATE from a training or gradient call
 * that would train a bunch of it: after bp_forward[_windows], bp_cv_chunk[_windows], bp_enhance_waves, bp_cv_mix, bp_eval_mix[_logmmse]
 * and a stream's push there are no targets on the device (bp_cv_* compare on the host; a stacked upload without targets leaves
 * an OLDER chunk's targets in the buffer).  bp_upload_chunk[_windows], bp_fill_chunk_synthetic, bp_train_*, bp_train_mix and
 * bp_mix_features (it makes the targets on the device) leave a chunk that can be trained on.  The handle is unchanged after
 * either error. */

/* ------------------------------------------------------------------------------------
 * On-device frame stacking.  The reference's reader materialises every
 * sample on the host as `context` consecutive normalised frames [+ the noise-aware block]
 * (Interface.cc:757-790) and uploads context x the raw volume.  Here the caller hands over the
 * RAW normalised frames of the chunk once plus three index tables; they STAY raw in device
 * memory and every bunch (training, CV, forward) stacks -- and, in training, dropout-masks -- its
 * own rows right before its layer-1 kernels: the stacked chunk is never materialised.  Row i of
 * the chunk, as the network sees it, is
 *     in[i]   = fea[win_start[i] .. win_start[i]+context)   (context*fea_dim contiguous floats)
 *               ++ nat[nat_row[i]]                          (fea_dim floats, only when nat != NULL)
 *     targ[i] = targ_frames[targ_frame[i]]                  (layersizes[L-1] floats)
 * i.e. bit-identical to what bp_upload_chunk would have received.  layersizes[0] must equal
 * context*fea_dim (+ fea_dim with a NAT block).  The caller may overwrite everything as soon
 * as the call returns. */
typedef struct bp_window_chunk {
    int n_samples;             /* rows (samples) of the chunk (<= chunk capacity) */
    int n_frames;              /* raw frames in fea / targ_frames */
    int fea_dim, context;
    int n_nat;                 /* rows of nat (0 when nat == NULL) */
    const float *fea;          /* [n_frames][fea_dim], already mean/variance normalised */
    const float *targ_frames;  /* [n_frames][layersizes[L-1]] */
    const float *nat;          /* [n_nat][fea_dim] or NULL */
    const int *win_start;      /* [n_samples] first raw frame of the window */
    const int *targ_frame;     /* [n_samples] raw frame whose target row is used */
    const int *nat_row;        /* [n_samples] or NULL */
} bp_window_chunk;
int bp_upload_chunk_windows(bp_handle *h, const bp_window_chunk *c);             /* then bp_train_resident etc. */
int bp_train_chunk_windows(bp_handle *h, const bp_window_chunk *c);              /* = BP_GPU::train on the stacked chunk */
int bp_cv_chunk_windows(bp_handle *h, const bp_window_chunk *c, float *sq_err_sum); /* = BP_GPU::CrossValid */
int bp_forward_windows(bp_handle *h, const bp_window_chunk *c, float *out);         /* = bp_forward: out[n_samples][sL] (enhancement) */

/* ------------------------------------------------------------------------------------
 * Waveform enhancement (no reference counterpart: the reference reads and writes log-power-spectrum Pfiles made by outside
 * tools).  One signal definition, derived from fea_dim: n_fft = 2*(fea_dim-1), a power of two from 64
 * to 2048 (else BP_ERR_ARG); hop = n_fft/2; periodic Hamming window w[k] = 0.54 - 0.46 cos(2 pi k / n_fft) for analysis and
 * synthesis; a sentence of n >= 1 samples is padded with n_fft-hop zeros in front and zeros behind and has
 * T = (n-1)/hop + 2 frames; samples are floats in int16 units; LPS = ln(max(|Y_k|^2, 1e-10)), k = 0 .. fea_dim-1.
 *
 * bp_enhance_waves: analysis -> (lps - mean) * inv_std -> the forward of bp_forward_windows on windows of `context` frames
 * whose output frame sits at targ_offset, the first and last frame of each sentence REPLICATED so that every frame gets an
 * output (bpforward drops edge windows instead) [+ the noise-aware block: mean of the sentence's first 6 normalised frames,
 * iff layersizes[0] == (context+1)*fea_dim] -> output columns o = [out_col, out_col+fea_dim) of the post-activation
 * output -> S = exp(o/2) Y/|Y| (BP_WAVE_LPS; phasor 1 where |Y| = 0) or S = o Y (BP_WAVE_MASK: amplitude gain) ->
 * least-squares overlap-add, sum_t w irfft(S_t) / sum_t w^2, trimmed to n samples.  out_pcm holds sum(sent_len) samples,
 * out_net (NULL or [sum T][layersizes[L-1]]) the net outputs per frame.  The frames of the call plus n_sent*(context-1)
 * replicated rows must fit the chunk capacity (max_chunk_frames).  The call becomes the handle's resident window chunk (as
 * after bp_forward_windows); training afterwards is unaffected.  Every argument is checked before the device is touched;
 * BP_ERR_STATE on a data-parallel-attached handle.  The same bits on every run.
 * bp_wave_lps: the analysis alone (no handle): lps[sum T][fea_dim], un-normalised. */
enum { BP_WAVE_LPS = 0, BP_WAVE_MASK = 1 };
typedef struct bp_wave_chunk {
    int n_sent; const int *sent_len; const float *pcm;   /* sentences back to back, int16 units */
    int context, targ_offset;                           /* as trained; NAT iff layersizes[0] == (context+1)*fea_dim */
    const float *mean, *inv_std;                        /* [fea_dim], the norm file */
    int target, out_col;                                /* BP_WAVE_LPS | BP_WAVE_MASK; first output column used */
} bp_wave_chunk;
int bp_enhance_waves(bp_handle *h, int fea_dim, const bp_wave_chunk *c, float *out_pcm, float *out_net);
int bp_wave_lps(int device, int fea_dim, int n_sent, const int *sent_len, const float *pcm, float *lps);

/* ------------------------------------------------------------------------------------
 * Training from clean speech and noise mixed on the device (no reference counterpart: the reference trains on Pfiles of
 * mixtures made offline by outside tools).  INTEGRATION.md 1e.  The signal definition of bp_enhance_waves applies unchanged.
 *
 * bp_set_mix_corpus uploads n_clean clean sentences and n_noise noise recordings (fp32 in int16 units, back to back, each at least
 * 1 sample long) plus the norm file, once; they stay resident on the handle until it is destroyed or the corpus is replaced.
 * target: BP_MIX_LPS | _IRM | _IBM | _LPS_IRM | _LPS_IBM (columns concatenated in that order); layersizes[L-1] must be fea_dim
 * (one part) or 2*fea_dim (two parts); layersizes[0] must be context*fea_dim or (context+1)*fea_dim (noise-aware block).
 *
 * A mixture {clean c, noise n, offset o, snr_db} (0 <= o < len(noise n), snr_db finite) of the clean sentence s (len_c samples):
 *   v[i] = noise_n[(o + i) mod len_n], i < len_c                       (the noise wraps)
 *   E_s = sum s^2, E_v = sum v^2, in double, fixed order; g = sqrt(E_s / (E_v 10^(snr_db/10))) in double rounded to fp32 once,
 *   g = 0 when E_v = 0;  x[i] = fmaf(g, v[i], s[i])
 * Features: the analysis of x, bit-identical to bp_wave_lps(x), normalised with mean / inv_std and stacked with replicated edge
 * frames [+ the noise-aware block] exactly as bp_enhance_waves stages them; every frame of every mixture is one sample.
 * Targets per frame, from S = analysis of s and N = analysis of the fp32 products g v[i]:
 *   LPS = ln(max(|S|^2, 1e-10)) (not normalised), IRM = sqrt(|S|^2 / max(|S|^2 + |N|^2, 1e-10)), IBM = (|S|^2 > 10^(lc_db/10) |N|^2).
 * Sample order: mixture-frame g runs over the frames of mixture 0, then mixture 1, ...  Row i of a call trains frame order[i]
 * (order == NULL: the identity; otherwise a permutation of [0, sum T)).  Capacity: sum T + n_mix*(context-1) <= max_chunk_frames.
 *
 * bp_train_mix = BP_GPU::train (bp_train_chunk_windows) on that chunk: consecutive full bunches, the partial last one ignored.
 * bp_cv_mix = BP_GPU::CrossValid (bp_cv_chunk_windows) on it in mixture-frame order: the same fp32 sum in the same order.
 * bp_mix_features: the chunk's data, unshuffled (any output may be NULL): fea [sum T][fea_dim] the normalised row of every frame
 * (as staged), lps [sum T][fea_dim] the noisy LPS, targ [sum T][layersizes[L-1]], nat [n_mix][fea_dim] (noise-aware nets only),
 * pcm [sum len_c] the mixed samples x.  Each of the three calls leaves the chunk as the handle's resident window chunk.
 * Every argument is checked before the device is touched (BP_ERR_ARG, the handle unchanged); BP_ERR_STATE without a corpus and
 * on a data-parallel-attached handle.  fp32 and bf16 handles.  No float atomics: the same bits on every run.
 *
 * Host only (no device), one definition for the command-line tool and Python.  philox(c0, c1, c2, c3) = the 4 output words of
 * Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and that counter; draws scale a word u to [0, n) as (u * n) >> 32.
 * bp_mix_plan: for mixture m = 0 .. n_clean*per_clean-1, u = philox(m, 0, 0, 0): clean = m / per_clean, noise = (u0 * n_noise)
 *   >> 32, offset = (u1 * noise_len[noise]) >> 32, snr_db = snr_db[(u2 * n_snr) >> 32].  Then the list is shuffled: for i from
 *   n-1 down to 1, j = (philox(i, 0, 1, 0)[0] * (i+1)) >> 32, swap entries i and j.  noise_len[k] in [1, 2^32).
 * bp_mix_shuffle: order = 0 .. n-1, then for i from n-1 down to 1, j = (philox(i, stream, 2, 0)[0] * (i+1)) >> 32, swap i and j. */
enum { BP_MIX_LPS = 0, BP_MIX_IRM = 1, BP_MIX_IBM = 2, BP_MIX_LPS_IRM = 3, BP_MIX_LPS_IBM = 4 };
typedef struct bp_mix_corpus {
    int fea_dim, context, targ_offset, target; float lc_db;
    const float *mean, *inv_std;                                   /* [fea_dim], the norm file */
    int n_clean; const int64_t *clean_len; const float *clean_pcm; /* back to back */
    int n_noise; const int64_t *noise_len; const float *noise_pcm;
} bp_mix_corpus;
typedef struct bp_mixture { int clean, noise; int64_t offset; float snr_db; } bp_mixture;
int bp_set_mix_corpus(bp_handle *h, const bp_mix_corpus *c);
int bp_train_mix(bp_handle *h, int n_mix, const bp_mixture *m, const int *order);
int bp_cv_mix(bp_handle *h, int n_mix, const bp_mixture *m, float *sq_err_sum);
int bp_mix_features(bp_handle *h, int n_mix, const bp_mixture *m, float *fea, float *lps, float *targ, float *nat, float *pcm);
int bp_mix_plan(uint64_t seed, int n_clean, int per_clean, int n_noise, const int64_t *noise_len, int n_snr, const float *snr_db,
                bp_mixture *out);
int bp_mix_shuffle(uint64_t seed, uint32_t stream, int n, int *order);

/* ------------------------------------------------------------------------------------
 * MFCC auxiliary target of the mixing corpus (multi-objective training: LPS, MFCC and a mask in one target row; no reference
 * counterpart).  INTEGRATION.md 1p.  The signal definition of bp_enhance_waves applies unchanged; M = fea_dim - 1.
 *
 * Two tables, computed on the host in double and rounded to fp32 once.
 * Filters: mel(f) = 2595 log10(1 + f/700).  Edges e_p, p = 0 .. n_mel+1: e_0 = f_lo and e_{n_mel+1} = f_hi as given, those between
 *   them equally spaced in mel between mel(f_lo) and mel(f_hi) and mapped back to Hz.  Bin k lies at f_k = k sample_rate / (2M).
 *   w[j][k] = max(0, min((f_k - e_j)/(e_{j+1} - e_j), (e_{j+2} - f_k)/(e_{j+2} - e_{j+1}))): triangles linear in Hz, not
 *   area-normalised.  first_bin[j], n_bins[j]: the bins with w[j][k] > 0 (after the rounding), a contiguous run.  A filter without
 *   such a bin is BP_ERR_ARG with a message that names it, from every call that takes the parameters together with a fea_dim.
 * DCT: t[r][j] = lift_i sqrt(2/n_mel) cos(pi i (j + 0.5)/n_mel), i = first_coef + r, lift_i = 1 + (L/2) sin(pi i/L) for the
 *   lifter L > 0, else 1 (HTK's).
 * Per frame, from P[k] = |S_k|^2 in fp32, S the analysis of the signal (as the LPS target's):
 *   E_j = sum_k (double)w[j][k] (double)P[k], k ascending from first_bin[j] over n_bins[j] bins, one double accumulator from +0.0;
 *   e_j = fl32(E_j);  logmel_j = e_j > 1e-10f ? logf(e_j) : ln(1e-10)                 (the floor of the LPS)
 *   c_r = fl32(sum_j (double)t[r][j] (double)logmel_j), j ascending, one double accumulator from +0.0
 *   target_r = (c_r - mean_r) * scale_r                                               in fp32
 * The product of two fp32 numbers is exact in double, so each step is one rounded double addition and the order is the
 * definition: e is a function of the bits of P and w, the target one of the bits of logmel, t, mean and scale.  A weight alpha_r on
 * the squared error of coefficient r needs nothing else: fold sqrt(alpha_r) into scale_r.
 *
 * bp_mel_defaults: 26 filters, 13 coefficients from c0, 0 .. sample_rate/2, L = 22, no mean / scale.
 * bp_mel_filters / bp_mel_dct (host only): the tables; any output of bp_mel_filters may be NULL.
 * bp_wave_mfcc (no handle, bp_wave_lps's frame plan): power [sum T][fea_dim], logmel [sum T][n_mel], mfcc [sum T][n_ceps] (mean
 *   and scale applied); any output may be NULL, not all three.
 * bp_set_mix_aux(h, p): p is checked and copied (NULL: off); it takes effect at the next bp_set_mix_corpus, where the tables are
 *   made for the corpus' fea_dim and uploaded -- a corpus that is already set keeps what it was set with.  With it the corpus
 *   target must begin with LPS (BP_MIX_LPS, _LPS_IRM, _LPS_IBM) and layersizes[L-1] must be parts*fea_dim + n_ceps: the target row
 *   is [LPS | MFCC | mask], the MFCC columns [fea_dim, fea_dim + n_ceps) bit-identical to bp_wave_mfcc of the entry's target
 *   signal (the early or reverberant signal of a derived entry).  Train with bp_set_output(h, 1, fea_dim +
 *   n_ceps, loss), enhance with out_col = fea_dim + n_ceps (mask) or 0 (LPS).  Without it nothing changes.  BP_ERR_ARG with the
 *   handle unchanged for a parameter outside the ranges below; BP_ERR_STATE on a data-parallel-attached handle. */
typedef struct bp_mel_params {
    int sample_rate;          /* Hz, > 0 */
    int n_mel;                /* 2 .. 128 */
    int n_ceps;               /* 1 .. n_mel - first_coef */
    int first_coef;           /* 0: c0 is the first column, 1: c1 is */
    float f_lo, f_hi;         /* 0 <= f_lo < f_hi <= sample_rate / 2 */
    float lifter;             /* HTK's L; 0: none */
    const float *mean, *scale;/* [n_ceps] or NULL (0 and 1): target = (c - mean) * scale */
} bp_mel_params;
int bp_mel_defaults(int sample_rate, bp_mel_params *p);
int bp_mel_filters(int fea_dim, const bp_mel_params *p, float *w /* [n_mel][fea_dim] */, int *first_bin, int *n_bins /* [n_mel] */);
int bp_mel_dct(const bp_mel_params *p, float *t /* [n_ceps][n_mel] */);
int bp_wave_mfcc(int device, int fea_dim, const bp_mel_params *p, int n_sent, const int *sent_len, const float *pcm,
                 float *power, float *logmel, float *mfcc);
int bp_set_mix_aux(bp_handle *h, const bp_mel_params *p);     /* NULL: off */

/* ------------------------------------------------------------------------------------
 * Reverberant entries of the mixing corpus (no reference counterpart).  INTEGRATION.md 1k.
 *
 * A room impulse response h has Lh taps, fp32 and finite, 1 <= Lh <= BP_MIX_RIR_MAX_TAPS.  Its delay d is the first index at
 * which |h[j]| is largest (bp_mix_rir_delay, host only).  For a clean sentence s of n samples, s[k] = 0 outside [0, n):
 *   acc_i(J) = sum_{j=0..J} (double)h[j] * (double)s[i + d - j]    added for j ascending, in double, starting from +0.0
 *   r[i] = fl32(acc_i(Lh - 1))                                      the reverberant sentence, n samples, aligned to the direct path
 *   e[i] = fl32(acc_i(min(Lh - 1, d + early_taps)))                 direct sound + early reflections (early_taps >= 0)
 * The product of two fp32 numbers is exact in double, so each step is one rounded double addition (fma or multiply-then-add:
 * the same bits); out-of-range terms are exact zeros and may be skipped.  The order over j is the definition.  h is not
 * normalised.
 *
 * bp_set_mix_reverb: pair k = {clean sentence pair_clean[k], response pair_rir[k]} becomes clean entry n_clean + k of the corpus
 * set by bp_set_mix_corpus, with the length of its clean sentence.  Its mixing signal is r; its target signal is r
 * (BP_REVERB_TARGET_REVERBERANT) or e (BP_REVERB_TARGET_EARLY).  The entries are made once per call on the device and stay
 * resident; a later bp_set_mix_reverb replaces them, bp_set_mix_corpus drops them.  Every mixing call (bp_train_mix, bp_cv_mix,
 * bp_mix_features, bp_eval_mix, bp_eval_mix_logmmse) then accepts bp_mixture.clean in [0, n_clean + n_pair).  The mixing
 * definition above holds with "clean sentence" read two ways: E_s, x = fmaf(g, v, s) and the noisy features use the mixing
 * signal; S, the LPS / IRM / IBM targets and the reference bp_eval_mix* scores against use the target signal.  Dry entries
 * [0, n_clean) are both signals at once and keep their bits.
 * BP_ERR_ARG before the device is touched, the handle unchanged: null pointers, n_rir < 1, n_pair < 1, a length outside
 * [1, BP_MIX_RIR_MAX_TAPS], a non-finite tap, a pair index out of range, a bad target, early_taps < 0.  BP_ERR_STATE without a
 * corpus or on a data-parallel-attached handle.  BP_ERR_NOMEM leaves the previous entries in place.
 *
 * bp_reverb_waves: the same kernel on caller-supplied sentences (sentence k of sent_len[k] >= 1 samples, back to back in pcm, with
 * response sent_rir[k]); out_rev / out_early [sum sent_len], either may be NULL (not both).  No handle: one host->device copy,
 * one launch, one device->host copy, one synchronisation.
 * bp_mix_reverb_pairs (host only): pair_rir[c] = (philox(c, 0, 3, 0)[0] * n_rir) >> 32 for c < n_clean. */
#define BP_MIX_RIR_MAX_TAPS 65536
enum { BP_REVERB_TARGET_REVERBERANT = 0, BP_REVERB_TARGET_EARLY = 1 };
typedef struct bp_mix_reverb {
    int n_rir; const int *rir_len; const float *rir_pcm;           /* back to back */
    int n_pair; const int *pair_clean, *pair_rir;
    int target, early_taps;
} bp_mix_reverb;
int bp_set_mix_reverb(bp_handle *h, const bp_mix_reverb *r);
int bp_reverb_waves(int device, int n_sent, const int *sent_len, const float *pcm, const int *sent_rir, int n_rir, const int *rir_len,
                    const float *rir_pcm, int early_taps, float *out_rev, float *out_early);
int bp_mix_rir_delay(const float *h, int n_taps, int *delay);
int bp_mix_reverb_pairs(uint64_t seed, int n_clean, int n_rir, int *pair_rir);

/* ------------------------------------------------------------------------------------
 * Simulated room impulse responses: the image-source model of a shoebox room (Allen & Berkley 1979) with windowed-sinc
 * fractional delays (Peterson 1986).  No reference counterpart.  INTEGRATION.md 1l, DESIGN.md 20.
 *
 * All arithmetic is in double; c = 343.0 m/s.  A room is a box L[0] x L[1] x L[2] metres with a source at src and a microphone
 * at mic; beta[2d] and beta[2d+1] are the reflection coefficients of the walls at coordinate 0 and at L[d] of axis d.  A response
 * has n_taps taps at sample_rate = fs and a delay window of window_taps = Tw samples.
 *   d0 = |src - mic| = sqrt((dx^2 + dy^2) + dz^2),  reach = (n_taps + Tw/2) c / fs,  N_d = ceil(reach / (2 L_d))
 *   images (n, p), n_d in [-N_d, N_d], p_d in {0, 1}:
 *     x_d = (1 - 2 p_d) src_d + 2 n_d L_d - mic_d,  dist = sqrt((x_0^2 + x_1^2) + x_2^2),  tau = dist fs / c
 *     a = ((B_0[n_0][p_0] B_1[n_1][p_1]) B_2[n_2][p_2]) (d0 / dist),  B_d[n][p] = beta[2d]^|n-p| beta[2d+1]^|n|
 *   h[j] = fl32( sum over the images of a w(j - tau) ),  j = 0 .. n_taps-1
 *     w(u) = 0.5 (1 + cos(2 pi u / Tw)) sinc(u) for |u| < Tw/2, else 0;  sinc(u) = sin(pi u) / (pi u), sinc(0) = 1
 * Each power of B_d is a repeated multiplication from 1.0 on the host (0^0 = 1); the device reads B_d as a table and calls no
 * pow.  The direct path has amplitude 1, so h peaks near tap round(d0 fs / c); h is not normalised otherwise (1k does not want
 * it).  Images whose window does not reach a tap add exact zeros to it and are skipped.
 * Order of one tap's sum: the images ascending in ((((n_2 + N_2) 2 + p_2) (2 N_1 + 1) + n_1 + N_1) 2 + p_1) (2 (2 N_0 + 1)) +
 * (n_0 + N_0) 2 + p_0, one double accumulator per tap starting from +0.0, no atomics and no sum across threads: the bits of a
 * response depend on its own room, length, fs and Tw only -- not on the other responses of the call, their order or the run.
 * The device evaluates w in a factored form: with m = rint(tau), f = tau - m and u = j - tau,
 * sin(pi u) = -(-1)^(j-m) sin(pi f) and cos(2 pi u / Tw) = cos(2 pi j / Tw) cos(2 pi tau / Tw) + sin(2 pi j / Tw) sin(2 pi tau / Tw),
 * so sin and cos are called per image and per tap, never per term; its distance from the formula above is a few double ulps of
 * the largest term.
 * The t60 of bp_rir_beta and bp_rir_rooms is NOMINAL: the image model of a shoebox decays more slowly than Eyring's formula
 * predicts (a float64 evaluation of a 5 x 4 x 3 m room gave a T20-fit decay of 0.30 s for nominal 0.20 s, 0.60 s for 0.40 s).
 * Limitation: 1k aligns a response at its LARGEST tap.  In long narrow rooms (8 x 2 x 2.4 m is one) a cluster of early
 * reflections can exceed the direct path; the reverberant sentence is then aligned to that cluster.
 *
 * bp_rir_image: response k for rooms[k] with rir_len[k] taps; out holds them back to back, the layout bp_mix_reverb.rir_pcm
 * takes.  One host->device copy, one launch, one device->host copy, one synchronisation; nothing global grows.
 * BP_ERR_ARG before the device is touched: n_rir < 1, null pointers, sample_rate outside [1000, 192000], window_taps outside
 * [2, 1024], a length outside [1, BP_MIX_RIR_MAX_TAPS], a non-finite field, L_d outside [0.5, 100], a position not strictly
 * inside the box, a beta outside [0, 1], d0 < 0.05, or (2 N_0 + 1)(2 N_1 + 1)(2 N_2 + 1) 8 > BP_RIR_MAX_IMAGES for a response
 * (the bound on how long one launch can run).
 * bp_rir_orders (host only): N_d and the number of images of the box, under the same checks except the last.
 * bp_rir_beta (host only): Eyring, alpha = 1 - exp(-((24 ln 10) / c) V / (S t60)), all six beta = sqrt(1 - alpha); V = (L_0 L_1) L_2,
 * S = 2 ((L_0 L_1 + L_0 L_2) + L_1 L_2); L_d in [0.5, 100], t60 > 0 and finite.
 * bp_rir_rooms (host only): n rooms from the seed, in the Philox convention of bp_mix_plan with third counter word 4:
 * U(r, a)[i] = philox(r, a, 4, 0)[i] / 2^32.  Room r: L_d = L_lo_d + U(r,0)[d] (L_hi_d - L_lo_d), t60 = t60_lo + U(r,0)[3]
 * (t60_hi - t60_lo), mic_d = margin + U(r,1)[d] (L_d - 2 margin), src the same from U(r, 2+k) for attempt k = 0 .. 31, the first
 * with dist_lo <= |src - mic| <= dist_hi (none: BP_ERR_ARG, the room named in the error string); beta = bp_rir_beta(L, t60).
 * BP_ERR_ARG: n < 1, null pointers, a non-finite field, lo > hi, L_lo_d < 0.5, L_hi_d > 100, t60_lo <= 0, margin <= 0,
 * 2 margin >= L_lo_d, dist_lo < 0.05.  Every room it returns passes the checks of bp_rir_image. */
#define BP_RIR_MAX_IMAGES (1 << 26)
typedef struct bp_rir_room { double L[3], src[3], mic[3], beta[6]; } bp_rir_room;
typedef struct bp_rir_range { double L_lo[3], L_hi[3], t60_lo, t60_hi, margin, dist_lo, dist_hi; } bp_rir_range;
int bp_rir_image(int device, int sample_rate, int window_taps, int n_rir, const bp_rir_room *rooms, const int *rir_len, float *out);
int bp_rir_orders(const bp_rir_room *r, int sample_rate, int n_taps, int window_taps, int order[3], int64_t *n_images);
int bp_rir_beta(const double L[3], double t60, double beta[6]);
int bp_rir_rooms(uint64_t seed, int n, const bp_rir_range *g, bp_rir_room *out);

/* ------------------------------------------------------------------------------------
 * Objective scores of enhanced speech (no reference counterpart: the papers it asks its users to cite score with outside tools).
 * INTEGRATION.md 1f.  Samples are fp32 in int16 units; a score compares an estimate e with a reference r of the same length n
 * at sample rate fs; eps = 2.220446049250313e-16; an undefined score is NaN, never an error.  Accepted rates: fs > 0 and
 * 10000/fs = p/q in lowest terms with max(p, q) <= 32 (8, 10, 12, 16, 20, 24, 32, 48 kHz), else BP_ERR_ARG.
 *
 * SSNR (dB; Hu & Loizou): win = floor(0.03 fs + 0.5), skip = floor(win/4), J = floor(n/skip - win/skip) frames (double; J < 1:
 *   NaN), w[i] = 0.5 (1 - cos(2 pi (i+1)/(win+1))), frame j at j skip, E_s = sum (w r)^2, E_d = sum (w (r - e))^2 in double,
 *   snr_j = clamp(10 log10(E_s/(E_d + eps) + eps), -10, 35), SSNR = mean_j snr_j.
 * LSD (dB): on the analysis of bp_wave_lps (fea_dim gives n_fft, hop, window, padding and the T frames), L = the fp32 LPS,
 *   LSD_t = sqrt((1/D) sum_k ((10/ln 10)(L_r - L_e))^2), LSD = mean_t LSD_t over all T frames (double).
 * STOI (Taal et al. 2011, with pystoi's guards): r and e resampled to 10 kHz unless fs = 10000 (scipy.signal.resample_poly(x, p,
 *   q): m = max(p, q), Lh = 10 m, h[j] = kaiser_{2Lh+1, 5}[j] sinc((j - Lh)/m) normalised to sum 1 times p, in double rounded
 *   once; y[k] = sum_j h[j] u[k q + Lh - j], u[t] = x[t/p] when p | t and 0 <= t/p < n; k < ceil(n p/q)); frames of N = 256 at
 *   K = 128 (every jK < n10 - N), symmetric Hann v[i] = 0.5 (1 - cos(2 pi (i+1)/(N+1))); frame j kept iff sum (v r)^2 >
 *   1e-4 max_j sum (v r)^2 (double); the kept frames of r and e (r's mask) overlap-added at cK, c = their rank (C kept);
 *   S = C - 1 STFT frames of v times the segment, zero-padded to 512; 15 one-third-octave band envelopes from 150 Hz (bins
 *   [7,9) [9,11) [11,14) [14,17) [17,22) [22,27) [27,34) [34,43) [43,55) [55,69) [69,87) [87,109) [109,138) [138,174) [174,219));
 *   S < 30: NaN; for m = 29 .. S-1 and each band, over x = X_b(m-29 .. m) and y likewise: alpha = sqrt(sum x^2/(sum y^2 + eps)),
 *   y' = min(alpha y, (1 + 10^0.75) x), rho = sum (x - mean x)(y' - mean y')/((|x - mean x| + eps)(|y' - mean y'| + eps));
 *   STOI = mean rho over the 15 (S - 29) pairs.
 *
 * bp_score_waves (no handle): n_sent pairs back to back in ref and est (equal lengths sent_len[s] >= 1) -> scores[n_sent][BP_SCORE_N].
 *   One host->device copy, one device->host copy, one synchronisation; every argument is checked before the device is touched.
 * bp_eval_mix: each mixture of the corpus set by bp_set_mix_corpus made exactly as bp_mix_features makes it, enhanced exactly as
 *   bp_enhance_waves would with target (BP_WAVE_LPS | BP_WAVE_MASK) and out_col, and both the mixed x and the enhanced samples
 *   scored against the clean s: noisy_scores[n_mix][BP_SCORE_N], enh_scores[n_mix][BP_SCORE_N], enh_pcm NULL or [sum len_c].  The
 *   audio stays on the device.  The argument checks and the capacity rule of bp_train_mix and bp_enhance_waves (BP_ERR_ARG, the
 *   handle unchanged); BP_ERR_STATE without a corpus and on a data-parallel-attached handle; fp32 and bf16 handles.  The call
 *   leaves the chunk as the resident window chunk; weights and momentum state are untouched.
 * Both: no float atomics, reductions in a fixed order -- the same bits on every run.
 *
 * The extended scores (the _ext calls with n_scores = BP_SCORE_EXT_N; two more columns behind the three above):
 * ESTOI (Jensen & Taal 2016): the STOI front end above unchanged up to the fp32 envelopes X_b(s) of r and Y_b(s) of e, b < 15,
 *   s < S; S < 30: NaN; for m = 29 .. S-1 the 15 x 30 matrices x[b][u] = X_b(m-29+u) and y likewise; on each matrix alone, in
 *   double: rows x[b][.] -= mean_u, x[b][.] /= (|x[b][.]| + eps), then columns x[.][u] -= mean_b, x[.][u] /= (|x[.][u]| + eps);
 *   d_m = (1/30) sum_{b,u} x[b][u] y[b][u]; ESTOI = mean d_m over the S - 29 segments.  No alpha scaling, no clipping, and no
 *   random dither (estoi.m and pystoi add eps randn; the + eps on the norms does that job here, as in the STOI above).
 * SI-SDR (dB; Le Roux et al. 2019), over the n samples in double: rr = sum r^2, er = sum e r; rr == 0: NaN; alpha = er/rr; in a
 *   second pass num = sum (alpha r_i)^2, den = sum (alpha r_i - e_i)^2 (the residual itself: sum e^2 - er^2/rr cancels at high
 *   SDR); SI-SDR = 10 log10(num/(den + eps) + eps).  The mean is not removed and nothing is clamped.
 *
 * The spectral-envelope scores (the _ext calls with n_scores = BP_SCORE_FULL_N; two more columns behind the five above):
 * LLR and cepstral distance CD (dB) (Hu & Loizou 2008; the REVERB challenge's set), on the SSNR's own framing: win, skip, the J
 *   frames and the window w above; P = 10 if fs < 10000, else 16; everything in double on the fp32 samples.  Per frame j and per
 *   signal x in {r, e}: xw[i] = w[i] x[j skip + i]; R_x[k] = sum_{i=0}^{win-1-k} xw[i] xw[i+k], k = 0..P (one fixed order of
 *   summation).  The frame is valid iff R_r[0] > 0 and R_e[0] > 0 (sums of squares: an exact decision).  White-noise correction:
 *   R_x[0] <- R_x[0] (1 + 1e-6).  Levinson-Durbin on the corrected R: E = R[0]; for m = 1..P: k = (R[m] - sum_{j=1}^{m-1} a[j]
 *   R[m-j])/E, a'[m] = k, a'[j] = a[j] - k a[m-j], E <- (1 - k^2) E; the prediction-error filter A = [1, -a_1 .. -a_P].  LPC
 *   cepstrum: c_1 = a_1, c_m = a_m + sum_{q=1}^{m-1} (q/m) c_q a_{m-q}, m <= P.  With T the (P+1) x (P+1) Toeplitz matrix of
 *   the corrected R_r: LLR_j = clamp(ln((A_e T A_e^T)/(A_r T A_r^T)), 0, 2), CD_j = clamp((10/ln 10) sqrt(2 sum_{m=1}^{P}
 *   (c_r[m] - c_e[m])^2), 0, 10).  Per sentence and per measure alone: Jv valid frames (Jv = 0 or J < 1: NaN), Jk = max(1,
 *   floor(0.95 Jv + 0.5)) (double); a valid frame is selected iff its rank #{valid i: v_i < v_j, or v_i == v_j and i < j} is
 *   below Jk (the doubles compared before any rounding); the score = (the sum of the selected values in one fixed order)/Jk,
 *   rounded once to fp32: Hu & Loizou's mean of the lowest 95 % with the tie rule stated.  The white-noise correction is not
 *   in Hu & Loizou's comp_llr, which has no guard: it keeps the Toeplitz system positive definite with condition <= (P+1) 1e6,
 *   so that the recursion never breaks down and no second, rounding-dependent validity decision exists.
 *
 * The critical-band scores (the _ext calls with n_scores = BP_SCORE_ALL_N; two more columns behind the seven above; sample_rate >=
 *   8000 and win <= 4096, else BP_ERR_ARG): the frequency-weighted segmental SNR fwSegSNR (dB) and the weighted spectral slope
 *   distance WSS (Hu & Loizou 2008; Klatt 1982), on the SSNR's own framing: win, skip, the J frames and the window w above; n_fft
 *   = 2^ceil(log2(2 win)), H = n_fft/2; everything in double on the fp32 samples, every sum in one fixed order.  This text is the
 *   definition (the published code was not at hand: the nearest-peak search below is how it is remembered).
 *   The bands, i = 0..24: centres cf (Hz) 50, 120, 190, 260, 330, 400, 470, 540, 617.372, 703.378, 798.717, 904.128, 1020.38,
 *   1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63; widths bw (Hz) 70
 *   (seven times), 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776, 217.153,
 *   235.631, 255.255, 276.072, 298.126, 321.465, 346.136; f0_i = cf_i/(fs/2) H, b_i = bw_i/(fs/2) H, g_i[k] = exp(-11 ((k -
 *   floor(f0_i))/b_i)^2) for k = 0..H-1, set to 0 where it is not greater than exp(-30/(2 2.303)).
 *   A frame is valid iff sum (w r)^2 > 0 and sum (w e)^2 > 0; an invalid frame is skipped.  R[k], E[k], k = 0..H-1: the n_fft-point
 *   DFTs of the windowed, zero-padded frames.
 *   fwSegSNR: a[k] = |R[k]|/sum_k |R[k]|, p[k] = |E[k]|/sum_k |E[k]|; c_i = sum_k g_i[k] a[k], d_i = sum_k g_i[k] p[k]; err_i =
 *   max((c_i - d_i)^2, 2^-52), W_i = c_i^0.2; v = sum_i W_i 10 log10(c_i^2/err_i) / sum_i W_i over the bands with c_i > 0 (none:
 *   the frame is invalid for this column); frame value min(max(v, -10), 35); the score = the mean over the valid frames, divided
 *   once, rounded once to fp32.  No trim.
 *   WSS: B_i = 10 log10(max(sum_k g_i[k] |R[k]|^2, 1e-10)), C_i likewise from E; slopes s_i = B_{i+1} - B_i, t_i = C_{i+1} - C_i,
 *   i = 0..23.  Nearest peak L_i: if s_i > 0: n = i; while n < 24 and s_n > 0: n++; L_i = B_{n-1} (the band below the summit);
 *   else: n = i; while n >= 0 and s_n <= 0: n--; L_i = B_{n+1}.  Wr_i = 20/(20 + max_j B_j - B_i) 1/(1 + L_i - B_i) (the max
 *   over all 25 bands), We_i likewise from C and t, W_i = (Wr_i + We_i)/2; frame value sum_i W_i (s_i - t_i)^2 / sum_i W_i; the
 *   score = the mean of the lowest 95 % of the valid frames under the rule of LLR / CD above (Jk, the tie rule), rounded once.
 *   A column is NaN when it has no valid frame.
 * Not computed: PESQ and the composite measures (no copy of P.862 to hold them to) and SRMR (non-intrusive).
 *
 * bp_score_waves_ext, bp_eval_mix_ext (and bp_eval_mix_logmmse_ext, bp_eval_mix_logmmse_nt below): the calls above with rows of
 *   n_scores columns, n_scores = BP_SCORE_N, BP_SCORE_EXT_N, BP_SCORE_FULL_N or BP_SCORE_ALL_N, anything else BP_ERR_ARG before
 *   the device is touched; every other check, state and capacity rule is that of the call without _ext.  With BP_SCORE_N an _ext
 *   call is that call; with BP_SCORE_EXT_N columns 0..2 hold its bits, and only then do the ESTOI and SI-SDR kernels run; with
 *   BP_SCORE_FULL_N columns 0..4 hold the bits of the five-column call, and only then do the LLR and CD kernels run; with
 *   BP_SCORE_ALL_N columns 0..6 hold the bits of the seven-column call, and only then do the fwSegSNR and WSS kernels run. */
enum { BP_SCORE_SSNR = 0, BP_SCORE_LSD = 1, BP_SCORE_STOI = 2, BP_SCORE_N = 3 };
enum { BP_SCORE_ESTOI = 3, BP_SCORE_SISDR = 4, BP_SCORE_EXT_N = 5 };
enum { BP_SCORE_LLR = 5, BP_SCORE_CD = 6, BP_SCORE_FULL_N = 7 };
enum { BP_SCORE_FWSSNR = 7, BP_SCORE_WSS = 8, BP_SCORE_ALL_N = 9 };
int bp_score_waves(int device, int fea_dim, int sample_rate, int n_sent, const int *sent_len, const float *ref, const float *est,
                   float *scores);
int bp_eval_mix(bp_handle *h, int n_mix, const bp_mixture *m, int sample_rate, int target, int out_col, float *noisy_scores,
                float *enh_scores, float *enh_pcm);
int bp_score_waves_ext(int device, int fea_dim, int sample_rate, int n_sent, const int *sent_len, const float *ref, const float *est,
                       int n_scores, float *scores);   /* [n_sent][n_scores] */
int bp_eval_mix_ext(bp_handle *h, int n_mix, const bp_mixture *m, int sample_rate, int target, int out_col, int n_scores,
                    float *noisy_scores, float *enh_scores, float *enh_pcm);

/* ------------------------------------------------------------------------------------
 * The classic baseline: the log-MMSE (Ephraim-Malah log-spectral-amplitude) enhancer, the column every results table of the papers
 * the reference asks its users to cite sets beside the DNN (the reference ships enh_wav_example/test3_ForestGump_logMMSE_enh.wav
 * for that comparison; it has no code for it).  INTEGRATION.md 1h.  The signal definition of bp_enhance_waves applies unchanged
 * (n_fft, hop, window, padding, the T frames, fp32 samples in int16 units); Y_t[k] is the fp32 spectrum of that analysis, D =
 * fea_dim bins.  Everything below runs in double on those fp32 values.
 *
 * bp_logmmse_params {alpha, mu, eta, xi_min_db, gamma_max, init_frames}; bp_logmmse_defaults writes 0.98, 0.98, 0.15, -25, 40, 6
 * (Loizou's logmmse); a NULL params pointer means the defaults.  Valid: 0 <= alpha < 1, 0 <= mu <= 1, eta finite,
 * -100 <= xi_min_db <= 0, gamma_max >= 1 and finite, init_frames >= 1; anything else is BP_ERR_ARG before the device is touched.
 *
 * Per sentence and per bin k, P_t = re^2 + im^2, xi_min = 10^(xi_min_db/10), lambda_floor = 1e-10 (the LPS floor):
 *   lambda = max(mean_{t < min(init_frames, T)} P_t, lambda_floor)     (the noise start: the sentence's first frames, as the
 *                                                                      noise-aware block takes them)
 *   for t = 0 .. T-1:
 *     gamma = min(P_t / lambda, gamma_max)
 *     xi    = (t == 0 ? alpha : alpha A_prev / lambda) + (1 - alpha) max(gamma - 1, 0);  xi = max(xi, xi_min)
 *     Lambda = gamma xi/(1+xi) - ln(1+xi)
 *     vad_t = (1/D) sum_k Lambda_k                                     (one fixed summation order)
 *     if vad_t < eta: lambda <- max(mu lambda + (1 - mu) P_t, lambda_floor)   (from frame t+1 on; frame t's gain uses the xi, gamma above)
 *     A = xi/(1+xi);  v = A gamma
 *     G = P_t > 0 ? A exp(E1(v)/2) : 0                                 (no clamp at 1: the usual form; G|Y| stays below about
 *                                                                      0.75 sqrt(A lambda))
 *     A_prev = G^2 P_t                                                 (G unrounded)
 *     S_t[k] = fl32(G) Y_t[k]
 * E1 is the exponential integral: for x <= 1, -gamma_E - ln x - sum_{n>=1} (-x)^n/(n n!) summed to convergence; for x > 1 the
 * continued fraction e^-x/(x+1 - 1/(x+3 - 4/(x+5 - ...))) by the modified Lentz method to 1e-16.
 * Synthesis and overlap-add are those of bp_enhance_waves with BP_WAVE_MASK and the gain row in place of the net's output, trimmed
 * to n samples.  No float atomics: the same bits on every run.
 *
 * bp_logmmse_waves (no handle): out_pcm holds sum(sent_len) samples; out_gain NULL or [sum T][fea_dim], fl32(G); out_vad NULL or
 *   [sum T], fl32(vad_t).  One host->device copy, one device->host copy, one synchronisation; every argument is checked before the
 *   device is touched.
 * bp_eval_mix_logmmse: bp_eval_mix with this enhancer in place of the net -- each mixture made exactly as bp_mix_features makes
 *   it, enhanced exactly as bp_logmmse_waves would enhance the mixed samples, x and the result scored against the clean s exactly
 *   as bp_eval_mix scores them; the audio stays on the device.  The argument and capacity rules of bp_eval_mix; BP_ERR_STATE
 *   without a corpus and on a data-parallel-attached handle.  The call leaves the chunk as the resident window chunk; weights and
 *   momentum state are untouched.  It does not run the net: it neither sizes nor writes the net's output block, whatever its size
 *   against the calls before it, and nothing reads that block for this chunk -- the chunk has no targets, so the calls that would
 *   run the net on it (bp_train_resident, bp_grads_resident, bp_profile_step) refuse it as a chunk without targets, and every
 *   query computes its own outputs afresh.  In BP_NAT_DYNAMIC the call still stages one noise-aware row per frame (the mixing sequence is
 *   bp_mix_features'); its scores do not read them.  bp_eval_mix_logmmse_ext: the same with rows of n_scores columns, as
 *   bp_eval_mix_ext has them. */
typedef struct bp_logmmse_params {
    double alpha;        /* decision-directed weight of the a-priori SNR */
    double mu;           /* smoothing of the noise update in frames the VAD calls noise */
    double eta;          /* VAD threshold on the mean log likelihood ratio */
    double xi_min_db;    /* floor of the a-priori SNR, dB */
    double gamma_max;    /* cap of the a-posteriori SNR */
    int    init_frames;  /* frames of the noise start */
} bp_logmmse_params;
int bp_logmmse_defaults(bp_logmmse_params *p);
int bp_logmmse_waves(int device, int fea_dim, const bp_logmmse_params *p, int n_sent, const int *sent_len, const float *pcm,
                     float *out_pcm, float *out_gain, float *out_vad);
int bp_eval_mix_logmmse(bp_handle *h, const bp_logmmse_params *p, int n_mix, const bp_mixture *m, int sample_rate,
                        float *noisy_scores, float *enh_scores, float *enh_pcm);
int bp_eval_mix_logmmse_ext(bp_handle *h, const bp_logmmse_params *p, int n_mix, const bp_mixture *m, int sample_rate,
                            int n_scores, float *noisy_scores, float *enh_scores, float *enh_pcm);

/* ------------------------------------------------------------------------------------
 * Streaming sessions: audio that is still arriving, enhanced in blocks (no reference counterpart).  INTEGRATION.md 1g.  The signal
 * definition of bp_enhance_waves applies unchanged, and a sentence pushed in blocks of ANY sizes returns the same bits as one
 * bp_enhance_waves call on the finished sentence on the same handle.
 *
 * A stream has n_chan independent channels (feeds); one bp_stream_push advances all of them.  n_in[ch] >= 0 new samples per channel,
 * back to back in channel order in pcm; end[ch] != 0 (end may be NULL) closes the channel's current sentence after these samples;
 * n_out[ch] and out_pcm return the samples that became final, back to back in channel order.  After end the channel has returned
 * exactly as many samples as it received and starts a new sentence with the next push; end on a channel that has received nothing
 * is a no-op.
 *
 * bp_stream_counts (host only): what a channel has produced after `received` samples of its sentence.  hop = fea_dim - 1,
 * la = context - 1 - targ_offset (the look-ahead), T = (received - 1)/hop + 2 (0 when nothing was received):
 *   frames_in  = ended ? T : received / hop           (frame t needs the real samples [(t-1) hop, (t+1) hop))
 *   the noise-aware row is known once frames_in >= 6, or at the end (nets without the block: always)
 *   frames_out = 0 until then, after that ended ? T : max(0, frames_in - la)
 *   samples_out = ended ? received : max(0, frames_out - 1) hop
 * A push returns samples_out(after) - samples_out(before) per channel; the latency of a live feed is (la + 1) hop samples plus
 * the block, and 6 hop at the start of a sentence of a noise-aware net.
 *
 * Every argument is checked before the device or the stream's state is touched; after an error the stream continues as if the
 * call had not happened.  BP_ERR_ARG: the checks of bp_enhance_waves, n_chan < 1, max_push_samples < 1, sum(n_in) >
 * max_push_samples, out_cap smaller than the samples due, or the rows of the push (frames to enhance + context-1 per active
 * channel) exceeding max_chunk_frames.  BP_ERR_STATE on a data-parallel-attached handle.  A handle may hold several streams;
 * bp_destroy releases those still open.  fp32 and bf16 handles, every output option of bp_set_output.  A push leaves its rows as the
 * handle's resident window chunk; training, bp_enhance_waves, bp_forward_windows and bp_eval_mix calls between pushes disturb
 * neither the stream nor themselves.  Per push: one host->device copy, one device->host copy, one synchronisation; everything is
 * allocated at bp_stream_open.  No float atomics: the same bits on every run. */
typedef struct bp_stream bp_stream;
typedef struct bp_stream_config {
    int fea_dim, context, targ_offset;      /* as bp_wave_chunk; NAT iff layersizes[0] == (context+1)*fea_dim */
    const float *mean, *inv_std;            /* [fea_dim], copied at open */
    int target, out_col;                    /* BP_WAVE_LPS | BP_WAVE_MASK; first output column used */
    int n_chan;                             /* independent channels (feeds) advanced by one push, >= 1 */
    int max_push_samples;                   /* upper bound of sum(n_in) of one push, >= 1 */
} bp_stream_config;
int bp_stream_open(bp_handle *h, const bp_stream_config *c, bp_stream **out);
int bp_stream_push(bp_stream *s, const int *n_in, const float *pcm, const unsigned char *end, int *n_out, float *out_pcm,
                   size_t out_cap);
int bp_stream_close(bp_stream *s);
/* 1 for a stream opened while its handle was in BP_FORWARD_ROWINV (it packs its channels, bp_set_forward), else 0 (null: 0) */
int bp_stream_packed(const bp_stream *s);
int bp_stream_counts(int fea_dim, int context, int targ_offset, int nat, int64_t received, int ended, int64_t *frames_in,
                     int64_t *frames_out, int64_t *samples_out);

/* ------------------------------------------------------------------------------------
 * Log-MMSE streams: the classic baseline on audio that is still arriving (no reference counterpart).  INTEGRATION.md 1j.  A
 * log-MMSE stream has no handle and no net: it is opened on a device ordinal, as bp_logmmse_waves is called on one, and a
 * sentence pushed in blocks of ANY sizes, on any channel, in any company, returns the same bits as
 * bp_logmmse_waves(device, fea_dim, p, 1, ...) on the finished sentence.
 *
 * Channels, pushes and ends are those of bp_stream_push: n_in[ch] >= 0 new samples per channel, back to back in channel order in
 * pcm; end[ch] != 0 (end may be NULL) closes the channel's sentence after these samples; n_out[ch] and out_pcm return the samples
 * that became final.  After end the channel has returned exactly as many samples as it received, and its next push starts a new
 * sentence from a fresh noise start; end on a channel that has received nothing is a no-op.
 *
 * bp_lmstream_counts (host only) is bp_stream_counts with look-ahead 0 and the noise start in place of the noise-aware row.
 * hop = fea_dim - 1, T = (received - 1)/hop + 2 (0 when nothing was received):
 *   frames_in  = ended ? T : received / hop
 *   the noise start (the mean power of the sentence's first min(init_frames, T) frames) is known once frames_in >= init_frames,
 *   or at the end
 *   frames_out = 0 until then, after that ended ? T : frames_in
 *   samples_out = ended ? received : max(0, frames_out - 1) hop
 * A push returns samples_out(after) - samples_out(before) per channel; the latency of a live feed is one hop plus the block, and
 * init_frames hops at the start of a sentence (until the noise start is known the samples wait on the host).
 *
 * Every argument is checked before the device or the stream's state is touched; after an error the stream continues as if the
 * call had not happened.  BP_ERR_ARG: the checks of bp_logmmse_waves (fea_dim, the parameter ranges, the device ordinal), n_chan
 * outside 1 .. 65536, max_push_samples < 1, a negative n_in, sum(n_in) > max_push_samples, a null pcm or out_pcm that is needed,
 * out_cap smaller than the samples due (bp_lmstream_counts: received < 0, a null output, init_frames < 1).  BP_ERR_NOMEM when the
 * allocations of bp_lmstream_open fail, or when one push could hold 2^31 samples.  Everything is allocated at open; per channel
 * that is 2 fea_dim doubles and hop floats of device state, (init_frames + 4) hop floats in each of the push's input block (device
 * and pinned host) and its output block (the same), and (init_frames + 2) hop floats of host carry; besides max_push_samples
 * floats in each of the four blocks.  A push that gives some channel a new output frame makes one host->device copy, ONE kernel
 * launch (one workgroup per such channel takes its new frames from PCM to PCM), one device->host copy and one synchronisation; a
 * push that gives none does not touch the device.  No float atomics: the same bits on every run.  The stream owns a non-blocking
 * HIP stream of its own; bp_lmstream_close is its only release (NULL: BP_OK).  Other calls on the device between pushes --
 * bp_logmmse_waves, a handle's training or enhancement, other streams -- disturb neither the stream nor themselves. */
typedef struct bp_lmstream bp_lmstream;
int bp_lmstream_open(int device, int fea_dim, const bp_logmmse_params *p, int n_chan, int max_push_samples, bp_lmstream **out);
int bp_lmstream_push(bp_lmstream *s, const int *n_in, const float *pcm, const unsigned char *end, int *n_out, float *out_pcm,
                     size_t out_cap);
int bp_lmstream_close(bp_lmstream *s);
int bp_lmstream_counts(int fea_dim, int init_frames, int64_t received, int ended, int64_t *frames_in, int64_t *frames_out,
                       int64_t *samples_out);

/* ------------------------------------------------------------------------------------
 * Noise tracking in the log-MMSE baseline: an MMSE-SPP estimator (Gerkmann and Hendriks, "Unbiased MMSE-based noise power estimation
 * with low complexity and low tracking delay", 2012) in place of the VAD-gated update, which freezes once the noise level rises
 * (no reference counterpart).  INTEGRATION.md 1n, DESIGN.md 26.  Everything of the log-MMSE definition above stays -- the signal
 * layer, P_t, lambda_floor = 1e-10, the noise start from the first min(init_frames, T) frames, gamma, xi, Lambda, vad_t, G, A_prev,
 * the synthesis -- but the noise update, which in tracker mode also moves IN FRONT OF the frame's gain.
 *
 * bp_noise_params {mode, xi_h1_db, q, a_pow, a_spp, p_lo, p_cap}; bp_noise_defaults writes BP_NOISE_SPP, 15, 0.5, 0.8, 0.9, 0.98,
 * 0.99 (the paper's constants); a NULL pointer means these defaults.  Valid: mode BP_NOISE_VAD or BP_NOISE_SPP, 0 <= xi_h1_db <= 40,
 * 0 < q < 1, 0 <= a_pow < 1, 0 <= a_spp < 1, 0 < p_lo < p_cap < 1; anything else is BP_ERR_ARG with a message that names the field,
 * before the device is touched.
 *
 * mode BP_NOISE_SPP, per sentence and per bin, in double; the host computes xi = 10^(xi_h1_db/10), c0 = (1-q)/q (1+xi),
 * c1 = xi/(1+xi); pbar = 0 at the start of every sentence:
 *   for t = 0 .. T-1:
 *     ph   = 1 / (1 + c0 exp(-c1 P_t / lambda))                        (speech presence probability under a fixed a-priori SNR)
 *     pbar = a_spp pbar + (1 - a_spp) ph
 *     r    = clamp((pbar - p_lo) / (p_cap - p_lo), 0, 1)
 *     ph   = min(ph, 1 - (1 - p_cap) r)                                (the anti-stagnation ceiling)
 *     lambda = max(a_pow lambda + (1 - a_pow) ((1 - ph) P_t + ph lambda), lambda_floor)
 *     noise_t = lambda
 *     gamma, xi (with alpha A_prev / lambda), Lambda, vad_t, G, A_prev, S_t as above, from this lambda
 *     (no VAD-gated update: mu and eta take no part; vad_t is still computed and returned)
 * One deliberate difference from the paper: it caps ph at 0.99 by a hard switch, pbar > 0.99.  On sustained tones pbar comes within
 * 3e-7 .. 3e-4 of 0.99, a flipped switch moves that bin's lambda by at least 1.7 % (ph > 0.99 needs P/lambda > 8.3), and so an fp32
 * analysis could not be held to a float64 restatement.  The ceiling here ramps from 1 at pbar = p_lo to p_cap at pbar >= p_cap:
 * the same cure, continuous.  Tracker mode contains no decision at all: min, max and clamp only.
 * mode BP_NOISE_VAD is the definition above unchanged: the _nt calls then return the bits of the calls without _nt.
 *
 * bp_logmmse_waves_nt, bp_eval_mix_logmmse_nt, bp_lmstream_open_nt: bp_logmmse_waves, bp_eval_mix_logmmse_ext and bp_lmstream_open
 * with the noise parameters np, and every rule of theirs.  out_noise is NULL or [sum T][fea_dim]: in tracker mode fl32(noise_t), in
 * VAD mode fl32 of the lambda that frame t's gamma used (row 0: the noise start).  bp_lmstream_push, _close and _counts serve both
 * kinds of stream unchanged; the noise start still gates a sentence's first output.  A stream in tracker mode carries pbar beside
 * lambda and A_prev: 3 fea_dim doubles and hop floats of device state per channel; a sentence's end resets it. */
enum { BP_NOISE_VAD = 0, BP_NOISE_SPP = 1 };
typedef struct bp_noise_params {
    int    mode;         /* BP_NOISE_VAD | BP_NOISE_SPP */
    double xi_h1_db;     /* the fixed a-priori SNR under speech presence, dB */
    double q;            /* the a-priori probability of speech absence */
    double a_pow;        /* smoothing of the noise power */
    double a_spp;        /* smoothing of the presence probability */
    double p_lo, p_cap;  /* the ceiling of ph ramps from 1 at pbar = p_lo to p_cap at pbar >= p_cap */
} bp_noise_params;
int bp_noise_defaults(bp_noise_params *p);
int bp_logmmse_waves_nt(int device, int fea_dim, const bp_logmmse_params *p, const bp_noise_params *np, int n_sent,
                        const int *sent_len, const float *pcm, float *out_pcm, float *out_gain, float *out_vad, float *out_noise);
int bp_eval_mix_logmmse_nt(bp_handle *h, const bp_logmmse_params *p, const bp_noise_params *np, int n_mix, const bp_mixture *m,
                           int sample_rate, int n_scores, float *noisy_scores, float *enh_scores, float *enh_pcm);
int bp_lmstream_open_nt(int device, int fea_dim, const bp_logmmse_params *p, const bp_noise_params *np, int n_chan,
                        int max_push_samples, bp_lmstream **out);

/* ------------------------------------------------------------------------------------
 * The dynamic noise-aware input: a tracked noise estimate per frame in place of one row per sentence (dynamic noise-aware
 * training, Xu, Du, Dai, Lee, Interspeech 2014; no counterpart in the reference's code).  INTEGRATION.md 1o, DESIGN.md 27.
 *
 * A net with the noise-aware block (layersizes[0] == (context+1)*fea_dim) gets in = window(t) ++ nat.  BP_NAT_STATIC (the default,
 * today's code path and bits): nat is one row per sentence, the mean of its first 6 normalised frames.  BP_NAT_DYNAMIC: one row per
 * frame, the noise PSD that the MMSE-SPP tracker above holds at that frame, as a normalised LPS row.  Per sentence of T frames and
 * per bin k, Y the noisy spectrum of the analysis (1d), np the parameters of bp_set_nat in the units of the tracker above:
 *   P_t    = |Y_t[k]|^2                                          in double, from the fp32 parts of Y: exact products, one rounding
 *   lambda = max((sum_{t < min(6,T)} P_t, ascending t) / min(6,T), 1e-10);   pbar = 0        (the noise start, init_frames = 6)
 *   for t = 0 .. T-1:
 *     the tracker's step of frame t (ph, pbar, r, the ceiling, lambda: the five lines of mode BP_NOISE_SPP above)
 *     nat[t][k] = (l - mean[k]) * inv_std[k],   l = fl32(lambda) > 1e-10f ? logf(fl32(lambda)) : ln(1e-10)     in fp32
 * Sample g of the window chunk -- frame t of sentence s -- gets in = window(t) ++ nat[t]; its table entry nat_row[g] is the global
 * frame index F_s + t, not s.  No decision anywhere (min, max and the clamp only).  De-normalised, the rows are the log of the
 * out_noise of bp_logmmse_waves_nt on the same PCM with default bp_logmmse_params: the same Y bits, the same tracker, the same fl32.
 *
 * bp_set_nat(h, mode, np): np NULL means bp_noise_defaults.  BP_ERR_ARG, with the handle unchanged and a message that names the
 * field, for a null handle, a mode that is neither constant, np->mode != BP_NOISE_SPP together with BP_NAT_DYNAMIC (the VAD-gated
 * update needs the gains of the log-MMSE recursion), and the range rules of bp_noise_params (checked in either mode).  The setter
 * does not know `context`: BP_NAT_DYNAMIC on a net WITHOUT the block (layersizes[0] == context*fea_dim) is the BP_ERR_ARG of the
 * first call that stages the block.  Those calls follow the mode from the next call on: bp_enhance_waves, bp_train_mix, bp_cv_mix,
 * bp_mix_features, bp_eval_mix and bp_eval_mix_ext.  In BP_NAT_DYNAMIC the `nat` output of bp_mix_features is [sum T][fea_dim], one
 * row per frame in the order of `fea`.  Calls that hand over their own rows do not read the mode (bp_upload_chunk*,
 * bp_train_chunk_windows, bp_cv_chunk_windows, bp_forward_windows: a caller passes one row per frame through bp_window_chunk.nat
 * and nat_row as it always could); neither do bp_eval_mix_logmmse* and the other calls without a net.
 * A stream keeps the mode and the parameters its handle had at bp_stream_open, as it keeps the forward's mode (default and packed
 * streams alike); a later bp_set_nat does not change open streams.  bp_stream_counts is unchanged: a dynamic stream is nat = 1, and
 * the noise start is what makes a sentence's first output wait for 6 frames.  A dynamic stream carries lambda and pbar,
 * 2 fea_dim doubles of device state per channel, across pushes; a sentence's end resets them.  Whatever the block sizes, a
 * finished sentence returns the bits of bp_enhance_waves in the same mode.
 * On an attached data-parallel handle every rank passes the same values, as for bp_set_output.  Additive: bp_abi_version stays 5. */
enum { BP_NAT_STATIC = 0, BP_NAT_DYNAMIC = 1 };
int bp_set_nat(bp_handle *h, int mode, const bp_noise_params *np);   /* np NULL: bp_noise_defaults */

/* ------------------------------------------------------------------------------------
 * Post-processing of the net's LPS estimate before resynthesis: global variance (GV) equalisation and mask gating (Xu, Du, Dai,
 * Lee, TASLP 2015 and Interspeech 2015; no counterpart in the reference's code).  INTEGRATION.md 1q, DESIGN.md 30.  Off by
 * default: without bp_set_post every entry point returns the bits it returned before.
 *
 * One post-processed value, per frame and bin k.  x: the LPS estimate, net output column out_col + k, post-activation; m: the mask
 * estimate, column mask_col + k; y: the noisy LPS of that frame and bin, with the bits of bp_wave_lps; c = gv_center[k],
 * s = gv_scale[k].  Every operation is fp32, rounded once, never contracted:
 *   1. GV, when gv is on:       d = x - c;  t = s * d;  x = c + t
 *   2. gate, when mask_col >= 0: hi > lo:  u = (m - lo) * inv, inv = (float)(1.0 / ((double)hi - (double)lo)) made once on the host,
 *                                          u = u > 0 ? (u < 1 ? u : 1) : 0                        (a NaN mask gives 0)
 *                                hi == lo: u = m >= hi ? 1 : 0
 *                                w = weight * u;  e = y - x;  q = w * e;  x = x + q
 * GV first, then the gate.  The value is what the synthesis takes in place of the net's column under BP_WAVE_LPS; out_net remains
 * the net's own outputs, and no post-processed row is written to memory by the enhancing calls.  lo = hi = theta, weight = 1 is the
 * hard rule (the noisy LPS where the mask reaches theta), weight = 0.5 the average of the two.
 *
 * bp_post_defaults: gv 0, arrays NULL, mask_col -1, mask_lo = mask_hi = 0.5, mask_weight 1.
 * bp_set_post(h, fea_dim, p): p NULL switches post-processing off.  Every argument is checked before the device is touched, and
 * on an error the handle is unchanged: BP_ERR_ARG for a null handle, 2 (fea_dim - 1) no power of two in 64 .. 2048, gv neither 0
 * nor 1, gv = 1 with a null array, a centre that is not finite, a scale that is not finite or not > 0, mask_col < -1 or mask_col +
 * fea_dim > layersizes[last], lo / hi / weight not finite, lo > hi, weight outside [0, 1]; BP_ERR_STATE on an attached
 * data-parallel handle.  The arrays are copied.  The parameters stay until the next call.  From then on bp_enhance_waves,
 * bp_eval_mix and bp_eval_mix_ext resynthesise from the post-processed value; they return BP_ERR_ARG, with nothing touched, when
 * the call's fea_dim differs from the one that was set, and when the target is BP_WAVE_MASK.  A stream copies the parameters when
 * it is opened (bp_stream_open makes the same two checks) and keeps them: a later bp_set_post does not change an open stream.
 * The log-MMSE calls, training and CV are unaffected.
 *
 * bp_post_rows (no handle): the same value over caller arrays, all [n_frames][fea_dim]; mask may be NULL when p->mask_col < 0 and
 * is otherwise the mask block itself (p->mask_col only switches the gate on).  out may be est.
 *
 * bp_gv_mix: the second moments that the GV factors are made from, over the mixtures of a plan, on the corpus and the handle state
 * of bp_eval_mix (fp32 and bf16 handles, both noise-aware modes; BP_ERR_STATE without a corpus).  For mixture-frame g = 0 .. n-1 of
 * the call and bin k:  e[g][k] = the net's column out_col + k (BP_GV_RAW) or the post-processed value (BP_GV_POST; identical to
 * BP_GV_RAW while post-processing is off);  r[g][k] = the LPS of the entry's clean target signal, the bits of bp_wave_lps on it.
 * Sum order, with q = (n + 63) / 64: part p = 0 .. 63 covers the frames [p q, min(n, (p+1) q)) and is one double accumulator from
 * 0.0 over ascending g, per bin and quantity -- the quantities (double)v and (double)v * (double)v, the product exact in double --
 * and the total is part 0 + part 1 + ... in ascending p (an empty part adds 0.0).  est_sum, est_sq, ref_sum, ref_sq [fea_dim] and
 * *frames (= n) are written, not added to: across calls the caller adds.  No float atomics; the same bits on every run.
 * bp_gv_mix leaves the chunk as the resident window chunk, without targets, as bp_eval_mix does; weights, momentum state and the
 * position of the dropout stream are untouched.
 *
 * bp_gv_factors (host only), in double: me = S1e / n, ve = S2e / n - me^2, and the same for r.  frames < 2 is BP_ERR_ARG; a
 * variance <= 0 (or not finite) is BP_ERR_ARG with the bin named in the message.  center[k] = (float)mr[k]: the paper scales in
 * the domain normalised by the clean statistics, which is scaling about the clean mean.  BP_GV_DEP: scale[k] =
 * (float)sqrt(vr[k] / ve[k]).  BP_GV_INDEP: every scale[k] = (float)sqrt(D / sum_k ve[k] / vr[k]), k ascending -- the paper's
 * dimension-independent factor, the variance of the estimate pooled over the bins after each is normalised by the clean mean and
 * deviation.  Additive: bp_abi_version stays 5. */
enum { BP_GV_RAW = 0, BP_GV_POST = 1 };        /* bp_gv_mix: the net's columns | the rows that are resynthesised */
enum { BP_GV_INDEP = 0, BP_GV_DEP = 1 };       /* bp_gv_factors: one factor for all bins | one per bin */
typedef struct bp_post_params {
    int gv;                                    /* 0 off | 1 on */
    const float *gv_center, *gv_scale;         /* [fea_dim], read when gv = 1; finite, scale > 0 */
    int mask_col;                              /* -1: no gating; else first column of the mask block in the net's output */
    float mask_lo, mask_hi, mask_weight;       /* finite, lo <= hi, 0 <= weight <= 1 */
} bp_post_params;
int bp_post_defaults(bp_post_params *p);       /* gv 0, mask_col -1, lo = hi = 0.5, weight 1 */
int bp_set_post(bp_handle *h, int fea_dim, const bp_post_params *p);     /* NULL: off.  Copies the arrays. */
int bp_post_rows(int device, int fea_dim, int n_frames, const float *est, const float *mask /* or NULL */,
                 const float *noisy_lps, const bp_post_params *p, float *out);               /* no handle; all [n_frames][fea_dim] */
int bp_gv_mix(bp_handle *h, int n_mix, const bp_mixture *m, int out_col, int stage,
              double *est_sum, double *est_sq, double *ref_sum, double *ref_sq /* [fea_dim] each */, int64_t *frames);
int bp_gv_factors(int fea_dim, int64_t frames, const double *est_sum, const double *est_sq, const double *ref_sum,
                  const double *ref_sq, int mode, float *center, float *scale);               /* host only */

/* ------------------------------------------------------------------------------------
 * Sample-rate conversion by a rational factor (no reference counterpart: its README sends its users to TIMIT at 16 kHz, NOISEX-92
 * at 19.98 kHz and 100 noise types at 20 kHz for nets that work at 8 kHz, and leaves the conversion to outside tools).
 * INTEGRATION.md 1m, DESIGN.md 24.  Defined to the bit, as the reverberation FIR above is.
 *
 * Ratio (bp_resample_ratio, host only): rate_out / rate_in = p / q in lowest terms.  Valid: both rates >= 1 and max(p, q) <= 1024
 * (44100 <-> 48000 is 160/147, 44100 -> 16000 is 160/441, 19980 -> 16000 is 800/999, 44100 -> 8000 is 80/441); anything else is
 * BP_ERR_ARG with the reduced ratio in the message.
 *
 * bp_resample_params {zeros, beta, rolloff}; bp_resample_defaults writes 16, 8.6, 0.9; a NULL params pointer means the defaults.
 * Valid: 1 <= zeros <= 32, 0 <= beta <= 20, 0 < rolloff <= 1; anything else is BP_ERR_ARG.
 *
 * Taps (bp_resample_taps, host only), made in double: with m = max(p, q) and Lh = zeros m, for j = 0 .. 2 Lh
 *   g[j] = I0(beta sqrt(1 - ((j - Lh) / Lh)^2)) / I0(beta) * sinc(rolloff (j - Lh) / m)
 *   h[j] = fl32(p g[j] / sum g)                                     the sum taken for j ascending
 * I0 is the modified Bessel function's power series sum_k ((x/2)^k / k!)^2 summed until a term no longer changes the sum;
 * sinc(u) = sin(pi u) / (pi u), sinc(0) = 1.  n_taps must be 2 zeros max(p, q) + 1.  The taps are fp32 on purpose: the product of
 * an fp32 tap and an fp32 sample is exact in double, so a fused multiply-add cannot change a bit of what follows.
 *
 * Output: a sentence x of n >= 1 samples gives n_out = ceil(n p / q) samples (bp_resample_len, host only, in int64):
 *   y[k] = fl32( sum_j (double)h[j] * (double)x[(k q + Lh - j) / p] )
 * over the j with p | (k q + Lh - j) and 0 <= (k q + Lh - j) / p < n, accumulated in double from +0.0 for j ascending, one term
 * after the other.  This is the placement of scipy.signal.resample_poly(x, p, q) with the filter's delay compensated; with
 * (zeros, beta, rolloff) = (10, 5, 1) it is the formula of the STOI resampler above.  rate_in == rate_out returns the bits of
 * the input and filters nothing.  Sentences never see each other's samples.  One lane owns one output sample: no float atomics and
 * no sum across lanes -- the same bits on every run, and for a sentence alone or in any company.
 *
 * bp_resample_waves (no handle): sentence s of sent_len[s] >= 1 samples, back to back in pcm; out holds sum n_out samples, back to
 * back.  One host->device copy, one launch, one device->host copy, one synchronisation (rate_in == rate_out: no device work).
 * Every argument is checked before the device is touched: BP_ERR_ARG for a bad ratio or parameter, n_sent < 1, null pointers, an
 * empty sentence, or 2^31 output samples or more in one call. */
typedef struct bp_resample_params {
    int    zeros;        /* zero crossings of the sinc on each side of its centre, counted at the lower of the two rates */
    double beta;         /* Kaiser window parameter */
    double rolloff;      /* cutoff as a fraction of the lower rate's Nyquist frequency */
} bp_resample_params;
int bp_resample_defaults(bp_resample_params *p);
int bp_resample_ratio(int rate_in, int rate_out, int *p, int *q);
int bp_resample_len(int64_t n, int p, int q, int64_t *n_out);
int bp_resample_taps(int p, int q, const bp_resample_params *params, float *h, int n_taps);
int bp_resample_waves(int device, int rate_in, int rate_out, const bp_resample_params *p, int n_sent, const int *sent_len,
                      const float *pcm, float *out);

/* ------------------------------------------------------------------------------------
 * Gradients without the update (parity tests; no reference counterpart -- the reference never
 * exposes layer_ydedx).  bp_grads_resident runs forward + backward of ONE local bunch starting at
 * chunk frame first_frame with the kernels of the data-parallel step and leaves the weight and bias
 * gradients (G_l = y_{l-1}^T . dEdX_l, BP_GPU.cu:642,647: sums over the bunch, not yet divided by n)
 * in a flat fp32 buffer [W_1 | b_1 | W_2 | b_2 ...] of padded rows (bp_grad_layout: offset/count of
 * layer l's segment; W_l is [pad64(prev)][pad64(cur)]); weights, momentum and the dropout stream
 * position stay untouched.  Not valid on an attached handle. */
int bp_grads_resident(bp_handle *h, int first_frame);
int bp_grad_floats(bp_handle *h, size_t *n_floats);
int bp_grad_layout(bp_handle *h, int layer, size_t *offset, size_t *count);
int bp_read_grads(bp_handle *h, float *host_dst, size_t n_floats);
/* Output y_l of hidden layer `layer` (1 .. numlayers-2; layer_y, BP_GPU.h:27: post-activation, post-dropout) for the
 * bunch processed last, [bunchsize][layersizes[layer]] floats.  Parity tests use it to count ReLU decisions that
 * fall within fp32 rounding of zero (they depend on the GEMM's summation order).  fp32 handles only. */
int bp_read_layer_output(bp_handle *h, int layer, float *host_dst, size_t n_floats);

/* ------------------------------------------------------------------------------------
 * In-library data-parallel exchange.  One process per GPU; each rank creates its handle
 * with bunchsize = frames of a minibatch it owns, global_bunchsize = world * bunchsize and
 * rank_frame_offset = rank * bunchsize, then joins the group.  `key` names the job (every rank passes the
 * same string, unique per job on the machine; a POSIX shared-memory block "/bpdp-<key>" carries the
 * rendezvous).  After bp_dp_attach, bp_train_resident / bp_train_chunk / bp_train_chunk_windows run
 * the data-parallel step on this rank's shard of every minibatch: per layer reduce-scatter of the
 * gradients (peer reads over xGMI through hipIpc mappings), momentum update of this rank's 1/world slice
 * of W and delta, all-gather of the new W (peer writes), ordered by device-side flags -- the semantics of
 * the reference's commented-out train_bunch_multi (BP_GPU.cu:775-908: gradient SUM, one update with
 * n = global bunch, identical weights everywhere) without routing through GPU 0.  No collective library
 * and no host synchronisation on the data path.  Every rank must make the same sequence of training
 * calls with the same number of minibatches.  Ranks may share a device (functional testing).
 * bp_get_weights works on every rank (weights are replicated); bp_get_deltas gathers the sharded momentum
 * state and must be called by all ranks together.  A rank that stops responding makes the others fail
 * with BP_ERR_STATE after BP_DP_TIMEOUT_S seconds (default 60) instead of hanging.  bp_set_hyper on an
 * attached handle must be given the same values by every rank.
 *
 * Before the first step relies on it, bp_dp_attach CHECKS the memory-model contract of the exchange on the
 * group's actual devices (peer write-through stores seen by the owner's cached loads; the owner's stores to
 * fine-grained memory seen by peers' system-scope loads), falls back to an explicit acquire behind every wait
 * if the first fails without one (bp_dp_peer_info reports the mode), and fails with BP_ERR_STATE otherwise.
 *
 * bp_dp_attach_ex selects the transport of the same sharded step: BP_DP_TRANSPORT_NATIVE (default: the peer
 * kernels above) or BP_DP_TRANSPORT_RCCL (ncclReduceScatter of every layer's gradient segment, the sharded
 * update, ncclAllGather of the new weights; librccl.so is loaded at run time; world 1, 2, 4 or 8; one rank
 * per device) or BP_DP_TRANSPORT_NATIVE_PUSH (round 6: the native exchange with the reduce-scatter turned round -- every rank
 * WRITES slice r of its gradient segment into rank r's receive buffer with write-through stores, the owner sums its world
 * local slots in the same fixed order; posted writes instead of peer reads on the fabric; same results bit for bit) or
 * BP_DP_TRANSPORT_NATIVE_PUSH_BF16 (the push form with every rank's contribution rounded to bf16 on the way out: half the bytes on the
 * fabric, fp32 summation at the owner in the same order; NOT the default for fp32 nets -- it changes results at the 1e-3 level,
 * tests/test_dp_native.py states and checks its tolerance). */
enum { BP_DP_TRANSPORT_NATIVE = 0, BP_DP_TRANSPORT_RCCL = 1, BP_DP_TRANSPORT_NATIVE_PUSH = 2, BP_DP_TRANSPORT_NATIVE_PUSH_BF16 = 3 };
int bp_dp_attach(bp_handle *h, int world, int rank, const char *key);
int bp_dp_attach_ex(bp_handle *h, int world, int rank, const char *key, int transport);
/* bp_dp_detach is collective.  Under more than one rank the momentum state is sharded (each rank updates its slices only), so a
 * bp_dp_detach whose barrier succeeded gathers it, as bp_get_deltas does, before it unmaps the peers: the detached handle holds
 * the whole momentum state, and bp_get_deltas, a checkpoint or a later bp_dp_attach of any transport continue from it.  bp_destroy
 * detaches too, without the gather (the state goes with the handle), and so does every failed path (a peer may be gone): after a
 * bp_dp_detach that returned an error the slices of the other ranks are stale.  EVERY rank of a group of more than one must call
 * bp_dp_detach itself: the gather meets the peers at two more barriers than the detach inside bp_destroy does, so a rank that
 * only destroys its handle no longer pairs up with a peer's bp_dp_detach -- that peer waits BP_DP_TIMEOUT_S and returns
 * BP_ERR_STATE, detached, with stale slices (ranks that ALL just call bp_destroy still pair up with each other). */
int bp_dp_detach(bp_handle *h);
int bp_dp_info(bp_handle *h, int *world, int *rank, unsigned *minibatches);
/* What rank `peer` of the group attached to: HIP device ordinal in ITS process and PCI bus id ("0000:c1:00.0";
 * buffer of >= 16 bytes), plus this group's transport and acquire mode (0 kernel boundary, 1 explicit acquire). */
int bp_dp_peer_info(bp_handle *h, int peer, int *device, char *pci_bus_id, int len, int *transport, int *acquire_mode);
/* How this group hands a layer's gradient segment to the exchange: 1 = inside the running weight-gradient launch (its tiles
 * count themselves behind system-scope write-through stores; native transport, bunches of 128 / 256 / 512 frames, fp32, at most
 * 4 weight layers = one grouped launch), 0 = event + kernel boundary per group of layers (RCCL, bf16, other bunch sizes, deeper
 * nets, or a group -- of one rank too -- whose attach-time self-test
 * found that form unusable on its devices, e.g. streams that do not run concurrently).  The same on every rank. */
int bp_dp_handoff(bp_handle *h, int *in_kernel);
/* Host-side barrier / all-gather of one small record (<= 64 bytes) per rank over the group's rendezvous block, for
 * launchers that have no other channel between the ranks (bench.py: barrier around the timed region, max over ranks). */
int bp_dp_barrier(bp_handle *h);
int bp_dp_allgather(bp_handle *h, const void *mine, size_t bytes, void *all);

/* The rendezvous underneath bp_dp_attach, usable on its own and WITHOUT a GPU (host code only): a POSIX
 * shared-memory block "/bpdp-<key>" created by rank 0, joined by ranks 1..world-1 within timeout_s, unlinked as
 * soon as everyone has joined (nothing is left behind by a later crash; a stale block of a crashed job with the
 * same key is ignored and replaced).  Replaces what the reference would need an MPI/NCCL bootstrap for; the
 * reference itself is single-process (BP_GPU.cu:29-36). */
typedef struct bp_rdv bp_rdv;
int bp_rdv_open(const char *key, int world, int rank, double timeout_s, bp_rdv **out);
int bp_rdv_barrier(bp_rdv *r);
int bp_rdv_allgather(bp_rdv *r, const void *mine, size_t bytes, void *all);   /* bytes <= 64 */
int bp_rdv_close(bp_rdv *r);
/* Pin / unpin caller-owned host memory (hipHostRegister) so that uploads from it (bp_train_chunk[_windows], bp_upload_*)
 * are DMA transfers instead of staged pageable copies; optional -- every entry point accepts pageable memory, which is what
 * the reference's callers have (`new[]`, Interface.cc:401-403; the reference stages through pinned memory itself,
 * BP_GPU.cu:926-992).  For hosts that do not link the HIP runtime. */
int bp_host_register(void *p, size_t bytes);
int bp_host_unregister(void *p);
/* PCI bus id of a visible device (hipDeviceGetPCIBusId), for hosts that do not link the HIP runtime. */
int bp_device_pci_bus_id(int device, char *buf, int len);

/* Timing of the dominant kernels for roofline reporting: average duration (ms) of the last
 * bp_train_resident call's whole bunch loop measured with HIP events on the handle's stream. */
int bp_last_train_ms(bp_handle *h, float *ms, int *bunches);
/* Time `iters` launches of one kernel of the step in isolation (HIP events on the handle's
 * stream).  which: 0 fwd hidden GEMM(layer 2), 1 dgrad hidden, 2 wgrad+update hidden,
 * 3 fwd layer 1, 4 fwd output layer, 5 wgrad+update layer 1.  Returns average ms.
 * bp_time_kernel leaves the weights, the momentum state, the resident chunk and the position of the dropout stream unchanged (ids
 * 2 and 5 update scratch copies of W, b and their deltas); it may overwrite the activations and the back-propagated errors of the
 * last bunch (what bp_read_layer_output returns), which every later call computes afresh before it reads them.  It runs on the
 * first bunchsize rows of a resident STACKED chunk, with or without targets (without: id 4 reads an older chunk's target rows,
 * which changes the time alone).  Refusals of bp_time_kernel, in this order: BP_ERR_ARG for a null argument, iters < 1, or ids 0..2
 * on a net without a hidden -> hidden layer; BP_ERR_STATE on a bf16 handle (the first of the state checks); BP_ERR_STATE when no
 * stacked chunk of at least bunchsize rows is resident; BP_ERR_ARG for an unknown id.  The handle is unchanged after each. */
int bp_time_kernel(bp_handle *h, int which, int iters, float *avg_ms);

/* The same bunch loop as bp_train_resident over n_bunches bunches with a HIP event recorded after every launch
 * on the launch stream: avg_ms[BP_PROF_*] = average duration of one launch of that class AS IT RUNS INSIDE THE
 * STEP (previous event -> own event, i.e. the kernel plus the dependent-launch boundary in front of it),
 * launches_per_step[] = how many launches of the class a step makes.  Trains like bp_train_resident does: the same bits in the
 * weights and the momentum state, the same advance of the dropout stream, the chunk left resident.
 * Refusals of bp_profile_step, in this order: BP_ERR_STATE on a bf16 or data-parallel handle (checked first), then the two of
 * bp_train_resident: a frame range outside the resident chunk (BP_ERR_ARG), a chunk without targets (BP_ERR_STATE). */
enum { BP_PROF_FWD_L1 = 0, BP_PROF_FWD_HIDDEN = 1, BP_PROF_FWD_OUT = 2 /* split-K GEMM with its reduce, one launch */, BP_PROF_DGRAD_OUT = 3,
       BP_PROF_DGRAD_HIDDEN = 4, BP_PROF_WGRAD = 5 /* every layer's wgrad + update: one grouped launch */, BP_PROF_KINDS = 6 };
int bp_profile_step(bp_handle *h, int first_frame, int n_bunches, float *avg_ms, int *launches_per_step);
/* Peaks measured on this device in this process: bare v_mfma_f32_32x32x2_f32 loop (TFLOP/s) and a float4
 * device copy of 1 GiB (GB/s, read + write bytes), to stand beside the vendor figures in a roofline report. */
int bp_measure_peaks(bp_handle *h, float *mfma_f32_tflops, float *hbm_copy_gbs);

/* ------------------------------------------------------------------------------------
 * Layer-wise pre-training of sigmoid nets: a stack of restricted Boltzmann machines trained with one-step contrastive
 * divergence (CD-1).  The reference has the slot (initwts_file) and fills it with random nets only (toolbox/weights/gen_rand_net).
 * INTEGRATION.md 1r, DESIGN.md 31.  fp32 throughout; sigma(x) = 1/(1+expf(-x)), the hidden activation 1 of bp_config.
 *
 * A stack has layer sizes s[0..L-1] as bp_config has them.  RBM l (1 <= l <= L-1) has V = s[l-1] visible and H = s[l] hidden
 * units: weights W_l [V][H] in the [prev][cur] layout of bp_create, hidden bias c_l [H] (the net's bias of layer l), visible
 * bias a_l [V] (the RBM's alone), and a momentum state dW, dc, da that starts at zero.  The input of RBM 1 is the caller's
 * stacked rows [n][s[0]], what bp_train_chunk takes as `in`; the input of RBM l > 1 is the mean-field output of RBMs 1 .. l-1
 * on those rows, x <- sigma(x W_j + c_j) for j = 1 .. l-1 (nothing is sampled there).
 *
 * One CD-1 step of RBM l on a bunch v0 [B][V] with {lrate, momentum, weightcost, visible, sample}:
 *   p0 = sigma(v0 W + c)
 *   s0 = sample ? (u < p0 ? 1 : 0) : p0          u[r][j] = (float)(word >> 8) * 2^-24   (exact in fp32; 0 <= u < 1)
 *   v1 = visible == 0 ? s0 W^T + a               (Gaussian visibles of unit variance: the inputs are mean/variance normalised)
 *                     : sigma(s0 W^T + a)        (Bernoulli visibles: the probability, not a sample)
 *   p1 = sigma(v1 W + c)
 *   gW = v1^T p1 - v0^T p0,  gc = sum_r (p1 - p0),  ga = sum_r (v1 - v0)             (sums over the bunch)
 *   d' = momentum d - lrate (g / B + wc w),  w' = w + d'        wc = weightcost for W and 0 for both biases
 *   recon = sum_r sum_i (v0 - v1)^2              the fp32 difference, squared and summed in double in a fixed order
 * word for row r and hidden unit j is word r & 3 of the Philox4x32-10 block with counter (idx_lo, idx_hi, l, t) and key
 * (seed_lo, seed_hi), idx = (r >> 2) H + j, t = the number of CD steps RBM l has APPLIED so far (the keying of the step's
 * dropout words with frame offset 0).  No float atomics, every summation order is fixed by the shapes: two stacks given the
 * same calls hold the same bits.
 *
 * bp_rbm_defaults (host only): layer 1 {visible 0, lrate 0.0005}, layers >= 2 {visible 1, lrate 0.01}; momentum 0.9, weightcost
 *   1e-5, sample 1 for both.  A new stack holds them.
 * bp_rbm_create: weights / hbias / vbias are indexed 1 .. numlayers-1 as in bp_create; vbias NULL or an entry NULL = zeros.  The
 *   stack allocates once, here: its parameters, one bunch of work space and room for max_chunk_frames rows (0 = BP_MAXCACHEFRAME).
 * bp_rbm_train_chunk: uploads the rows and runs one CD-1 step per consecutive full bunch (propagating up first when layer > 1);
 *   rows short of a bunch at the end train nothing, as in BP_GPU::train.  *recon_sq_sum (may be NULL) = the sum of the bunches'
 *   recon, each with the weights that bunch saw.
 * bp_rbm_up: out[n][s[layer]] = the mean-field output of RBM `layer` for every row, the rows short of a bunch included.
 * bp_rbm_step: the parity entry, one bunch.  Whatever the trace asks for comes back (any pointer may be NULL, and so may the
 *   trace); gw / gc / ga are the STORED gradients.  apply = 0: nothing of the stack changes -- not the weights, not the momentum
 *   state, not the counter.  apply = 1: it does to the stack exactly what bp_rbm_train_chunk does for that bunch.
 * bp_rbm_steps: the CD steps RBM `layer` has applied.  bp_rbm_get: the parameters (NULL arrays and NULL entries are skipped).
 * BP_ERR_ARG before the device is touched, the stack unchanged: null pointers, numlayers outside [2, BP_MAXLAYER], a size or the
 * bunch < 1, layer outside [1, numlayers-1], n_frames negative or over the capacity, lrate or weightcost negative or not
 * finite, momentum outside [0, 1), visible or sample not 0/1.
 * Out of scope: CD-k and persistent CD, sampled visibles, sparsity targets, bf16, data-parallel pre-training. */
typedef struct bp_rbm bp_rbm;
typedef struct bp_rbm_config {
    int device, numlayers;
    int layersizes[BP_MAXLAYER];
    int bunchsize, max_chunk_frames;
    uint64_t seed;
} bp_rbm_config;
typedef struct bp_rbm_hyper { float lrate, momentum, weightcost; int visible, sample; } bp_rbm_hyper;
typedef struct bp_rbm_trace {
    float *v0, *p0, *s0, *v1, *p1;   /* [B][V] or [B][H]; any may be NULL */
    float *gw, *gc, *ga;             /* [V][H], [H], [V] */
    double *recon;
} bp_rbm_trace;
int bp_rbm_defaults(int layer, bp_rbm_hyper *out);
int bp_rbm_create(const bp_rbm_config *cfg, const float *const *weights, const float *const *hbias, const float *const *vbias,
                  bp_rbm **out);
int bp_rbm_destroy(bp_rbm *s);
int bp_rbm_set_hyper(bp_rbm *s, int layer, const bp_rbm_hyper *p);
int bp_rbm_train_chunk(bp_rbm *s, int layer, int n_frames, const float *in, double *recon_sq_sum);
int bp_rbm_up(bp_rbm *s, int layer, int n_frames, const float *in, float *out /* [n][s[layer]] */);
int bp_rbm_step(bp_rbm *s, int layer, const float *in /* [bunchsize][s[0]] */, int apply, const bp_rbm_trace *trace);
int bp_rbm_steps(bp_rbm *s, int layer, unsigned *applied);
int bp_rbm_get(bp_rbm *s, float *const *weights, float *const *hbias, float *const *vbias);

#ifdef __cplusplus
}
#endif
#endif /* BP_C_API_H */
