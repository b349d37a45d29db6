// bp_handle.h -- what the translation units of libbp_hip.so share: the device state of one BP_GPU replacement object
// (bp_handle), error plumbing, and the "step operations" that bp_step.hip exports to the data-parallel driver
// (bp_dp.hip) and the measurement entry points (bp_profile.hip).  Internal: nothing in here is part of the C ABI
// (include/bp_c_api.h).
//
//   bp_step.hip      handle construction, chunk interface, every kernel launch of the training / CV / forward step
//   bp_dp.hip        in-library data-parallel exchange (rendezvous, hipIpc peers, RCCL transport, the sharded step driver)
//   bp_profile.hip   in-step event profile, measured peaks, isolated kernel timing
//   bp_wave.hip      the signal layer: STFT analysis into a window chunk, overlap-add resynthesis (bp_enhance_waves, bp_wave_lps), the
//                    noise-aware rows (bp_set_nat), post-processing of the LPS estimate (bp_set_post) and the MFCC kernel (bp_wave_mfcc)
//   bp_resample.hip  rational sample-rate conversion (bp_resample_waves, bp_resample_*; bp_resample.h)
//   bp_mix.hip       training mixtures made on the device from a resident clean + noise corpus (bp_set_mix_corpus, bp_train_mix, ...),
//                    and the calls that score or measure on those mixtures (bp_eval_mix*, bp_gv_mix)
//   bp_room.hip      room acoustics: sentences convolved with room impulse responses (bp_reverb_waves; bp_room.h for bp_set_mix_reverb)
//                    and the responses simulated with the image method (bp_rir_image, bp_rir_*)
//   bp_eval.hip      objective scores: segmental SNR, log-spectral distortion, STOI (bp_score_waves; bp_eval.h)
//   bp_stream.hip    streaming sessions: live audio enhanced in blocks, bit-identical to bp_enhance_waves (bp_stream_open, _push, ...)
//   bp_classic.hip   the classic baseline: the log-MMSE enhancer on the same signal layer (bp_logmmse_waves; bp_classic.h) and its
//                    streams (bp_lmstream_open, _push, ...)
//   bp_infer.hip     the row-invariant inference forward (bp_set_forward: BP_FORWARD_ROWINV), one thin-M kernel per layer
//   bp_rbm.hip       layer-wise pre-training: a stack of RBMs trained with CD-1 (bp_rbm_create, ...; its own handle, bp_rbm.h); it
//                    shares bp_mem.h and bp_device.h with the other units, no state
//   (bp_fft.h: the device functions and the frame plan of the signal-layer units; bp_stream_core.h: counts, carry, push checks and
//   the block owner of the two streaming engines; bp_mel.h: the tables and the launcher of the MFCC auxiliary target;
//   bp_philox_host.h: Philox on the host, for the planners of bp_mix.hip and bp_room.hip;
//   bp_mem.h: the holders that free device memory, pinned memory, events and streams, the grow-only policy, block layouts,
//   and fail / HIPCHK; bp_chunk.h: the resident chunk -- bp_handle::res --, how one becomes resident and what its readers check)
//
// Device layout (all fp32 unless a bf16 copy is named): every layer width s_l is padded to ld_l = roundup(s_l, 64); pad
// columns/rows are zero and stay zero under the step (DESIGN.md "padding invariants"), so the GEMM tiles never need
// column predicates and every row is 256-byte aligned.
//   W_l   [ld_{l-1}][ld_l]   (reference layout weights[l][p*cur+c], BP_GPU.cu:139)
//   y_l   [B][ld_l]          post-activation, post-dropout output of layer l (layer_y)
//   dx_l  [B][ld_l]          dE/dx of layer l (layer_dedx); layer_x/dydx/dedy are never stored
//   in    [cap][ld_0], targ [cap][ld_{L-1}]   resident stacked chunk (res.in() / res.targ(), bp_chunk.h)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "../../include/bp_c_api.h"
#include "bp_mem.h"
#include "bp_chunk.h"

typedef uint16_t bf16_t;

static inline int pad64(int x) { return (x + 63) & ~63; }

// Development switches (A/B aids of the measurements quoted in DESIGN.md): environment variables that only a library
// built with -DBP_DEV (`make dev` -> libbp_hip_dev.so, loaded through BP_HIP_LIB) reads.  The shipped library has ONE
// code path per shape and reads no environment except BP_DP_TIMEOUT_S and BP_WGRAD_SLOTS (bp_create).
#ifdef BP_DEV
static inline bool dev_flag(const char *name) { return getenv(name) != nullptr; }
static inline int dev_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
#endif

struct StepProf;
struct bp_dp;

// Checked noise parameters in the units the kernels use: c0 = (1-q)/q (1+xi), c1 = xi/(1+xi), xi = 10^(xi_h1_db / 10) (noise_check,
// bp_classic.h).  spp == false: the VAD-gated update of the log-MMSE recursion, and nothing else of this is read.
struct NoiseP { bool spp; double c0, c1, a_pow, a_spp, p_lo, p_cap; };

// Checked parameters of the MFCC auxiliary target (mel_check, bp_mel.h): bp_mel_params within its ranges, mean / scale copied
// (NULL: 0 and 1)
constexpr int MEL_MAX = 128;                                     // the most filters, and so the most coefficients
struct MelP {
    int sample_rate, n_mel, n_ceps, first_coef;
    double f_lo, f_hi, lifter;
    float mean[MEL_MAX], scale[MEL_MAX];
};

// Checked post-processing parameters (bp_set_post; post_check, bp_wave.hip) as the kernels take them: gate = mask_col >= 0,
// inv = (float)(1 / (hi - lo)) made in double (hi > lo), c / s the centre and the scale on the device (read when gv)
constexpr int POST_MAX_D = 1025;                                 // the largest fea_dim
constexpr int GV_PARTS = 64;                                     // parts of a bp_gv_mix sum
struct PostP { int gv, gate, mask_col; float lo, hi, inv, weight; const float *c, *s; };

struct bp_handle {
    bp_config cfg;
    int L;                       // number of layer sizes
    int s[BP_MAXLAYER], ld[BP_MAXLAYER];
    int B, Bg;                   // local / global bunch
    int cap;                     // rows a chunk may have (max_chunk_frames)
    // (the holders of a handle go with `delete h`, in reverse order of declaration: the two streams it owns are declared first
    // and so go last, after everything that was used on them)
    Stream own_stream, copy_stream;   // copy_stream: see "Upload path" below
    hipStream_t stream;               // the launch stream (= own_stream)
    int wgrad_slots;             // workgroups of the persistent weight-gradient launch (4 per CU; BP_WGRAD_SLOTS at creation)
    // parameters and momentum state live in two flat arenas with the layout of the flat gradient buffer
    // ([W_1|b_1|W_2|b_2|...], padded; g_off/g_cnt) so that data-parallel ranks can export them as ONE hipIpc
    // allocation each and the sharded update is a flat elementwise pass (bp_dp.h); W/b/dW/db point into them
    float *params, *deltas;
    float *W[BP_MAXLAYER], *b[BP_MAXLAYER], *dW[BP_MAXLAYER], *db[BP_MAXLAYER];
    bp_dp *dp;                   // attached data-parallel group (bp_dp_attach) or null
    StepProf *prof;              // bp_profile_step in progress: an event after every launch of the step
    const uint8_t *inj_mask[BP_MAXLAYER];   // bp_train_resident_masked in progress: device masks of this bunch per layer output
    const float *inj_x0;                    // ... and the masked copy of its input rows
    float *y[BP_MAXLAYER], *dx[BP_MAXLAYER];
    float *out_dev;
    float *slabs; size_t slab_stride; int out_splits;   // split-K workspace of the output layer
    unsigned *out_ticket;                               // ... and its ticket words (one per 32 x 32 output tile)
    float *grad; size_t grad_floats; size_t g_off[BP_MAXLAYER], g_cnt[BP_MAXLAYER];
    Buf host_out;                // pinned staging for CV outputs (grow-only, whole chunk)
    Buf out_chunk;               // device: network outputs of a whole chunk [frames][ld_L] (CV / forward), grow-only
    size_t out_chunk_frames;     // (both through out_chunk_reserve)
    uint32_t step;               // bunches trained so far (dropout stream position)
    uint32_t th_vis, th_hid;
    int fwd_mode;                     // bp_set_forward: the kernels of the inference forward (BP_FORWARD_DEFAULT | BP_FORWARD_ROWINV)
    float *inf_slab; unsigned *inf_ticket[BP_MAXLAYER];   // ROWINV: k-slice slabs (shared by the layers) and each layer's ticket words, or null
    int nat_mode; NoiseP nat_np;      // bp_set_nat: the noise-aware block of the calls that stage it (BP_NAT_STATIC | BP_NAT_DYNAMIC) and the tracker of the latter
    int out_act, out_lin, out_loss;   // output layer (bp_set_output): 0 linear | 1 logistic on columns [out_lin, s_L), loss of those columns
    Event ev0, ev1; float last_ms; int last_bunches;
    std::vector<Buf> allocs;     // everything dev_alloc handed out: lives as long as the handle
    // Upload path: host->device copies run on copy_stream so that chunk i+1 is uploaded while chunk i trains.  What is resident,
    // the two copies of each kind of chunk, the staged tiles and the events of the upload: bp_chunk.h
    Resident res;
    // compute_dtype == 1 (bp_bf16.h): bf16 copies, each in both orientations
    bool bf;
    int Bp;                                                  // bunch rows rounded up to 64
    bf16_t *Wb[BP_MAXLAYER];                                 // ONE bf16 shadow of the weights, [prev][cur] (the forward reads it through the LDS transpose read)
    bf16_t *yb[BP_MAXLAYER], *ybT[BP_MAXLAYER];              // [Bp][ld_l], [ld_l][Bp]   (l = 0: the input bunch)
    bf16_t *dxb[BP_MAXLAYER], *dxbT[BP_MAXLAYER];
    float *bf_ks_slab; unsigned *bf_ks_cnt;                  // split-k output forward (bp_bf16.h, KS): partial tiles and ticket words, or null
    // bp_enhance_waves (bp_wave.hip), grow-only: device input block, noisy spectrum, synthesis frames, padded output samples;
    // pinned host staging of the input block and of the output samples
    Buf wave[4], wave_pin[2];
    // bp_set_mix_corpus (bp_mix.hip): the resident corpus and the grow-only buffers of the mixing calls, or null
    struct MixState *mix;
    // bp_set_mix_aux (bp_mix.hip, bp_mel.h): the MFCC auxiliary target the next bp_set_mix_corpus is set with (checked parameters, or
    // aux_on) and the device block its tables go to, allocated once at the parameter limits
    bool aux_on; MelP aux; float *aux_tab;
    // bp_set_post (bp_wave.hip): post-processing of the LPS estimate in the calls that resynthesise (post_on: for this fea_dim, with
    // these parameters); post_tab: the device block of centre | scale, POST_MAX_D floats each, made by the first call that turns it on
    bool post_on; int post_D; PostP post; float *post_tab;
    // bp_gv_mix (bp_mix.hip): the part sums [GV_PARTS][4][POST_MAX_D] and behind them the totals [4][POST_MAX_D], in double; made
    // on first use
    float *gv_parts;
    // bp_stream_open (bp_stream.hip): the open streaming sessions of this handle
    std::vector<struct bp_stream *> streams;
};

// Coefficients of the momentum update (update_delta, bp_device.h; DevFunc.cu:313-318 for momentum_rule 0, :306-311 for 1):
// c1 = (1-m)*lr or lr, ndiv = the global bunch, rdiv = exact_rdiv(ndiv).
//
// exact_rdiv: 1/ndiv where multiplying by it IS the division -- ndiv a power of two and 1/ndiv a normal float: g * rdiv is then
// the correctly rounded g / ndiv for every float g, subnormal quotients included (both are g with its exponent moved, rounded
// once) -- and 0 for every other divisor (3, 96, 100: about 30 % of the words differ), for 0, negative and non-finite ones.  The
// kernels take rdiv != 0 as "multiply" (update_delta<true>, bp_device.h) and keep the IEEE division otherwise.
static inline float exact_rdiv(float ndiv)
{
    int ex;
    if (!(ndiv > 0.0f) || frexpf(ndiv, &ex) != 0.5f) return 0.0f;      // (frexpf of inf / NaN is not 0.5)
    const float r = 1.0f / ndiv;
    return r >= 1.17549435e-38f && r <= 3.40282347e+38f ? r : 0.0f;    // (2^127: the reciprocal is subnormal; below 2^-127: infinite)
}
struct UpdateCoef { float mom, c1, wc, ndiv, rdiv; };
static inline UpdateCoef update_coef(const bp_handle *h)
{
    const float m = h->cfg.momentum, lr = h->cfg.lrate;
    return {m, h->cfg.momentum_rule == 1 ? lr : (1 - m) * lr, h->cfg.weightcost, (float)h->Bg, exact_rdiv((float)h->Bg)};
}

// Every device buffer gets SLACK floats of zeroed tail so that whole-tile reads of the GEMM loaders (no predicates,
// see GemmArgs) stay inside the allocation.
static const size_t SLACK = 4096;
int dev_alloc(bp_handle *h, float **p, size_t n_floats);

// bp_profile_step: one HIP event after every launch of the step on the launch stream; the duration attributed to a
// launch is the time between the previous event and its own (= kernel + the dependent-launch boundary in front of it).
struct StepProf {
    std::vector<Event> ev; std::vector<int> kind; size_t used;
};

// ------------------------------------------------------------------ calls without a handle
// BP_OK once `device` is a valid ordinal and current
static inline int use_device(const char *who, int device)
{
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(BP_ERR_ARG, std::string(who) + ": device ordinal out of range");
    HIPCHK(hipSetDevice(device));
    return BP_OK;
}
// The device side of a one-shot call (bp_wave_lps, bp_logmmse_waves, bp_score_waves, bp_reverb_waves): a stream and one device
// block, both freed when the holder goes.  e is sticky: the call chains its copies and launches with `if (e == hipSuccess) e = ...`,
// finish() synchronises and turns the first error into BP_ERR_DEVICE "<who>: <hip error string>".
struct OneShot {
    Stream st;
    Buf d;
    hipError_t e = hipSuccess;
    int open(const char *who, int device, size_t bytes)
    {
        { const int r = use_device(who, device); if (r != BP_OK) return r; }
        e = st.create(hipStreamNonBlocking);
        if (e == hipSuccess) e = d.alloc(bytes);
        return BP_OK;
    }
    int finish(const char *who)
    {
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        return e == hipSuccess ? BP_OK : fail(BP_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
};

// ------------------------------------------------------------------ step operations (bp_step.hip)
// One bunch starting at chunk frame `first`: forward + backward; fused: momentum update inside the wgrad epilogues
// (train_bunch_single, BP_GPU.cu:484-673), else gradients to the flat buffer.
hipError_t bunch(bp_handle *h, int first, bool fused);
// nb fused bunches from chunk frame `first` (dp_bunch on an attached handle): the one place that sets next_first, advances
// h->step (per enqueued bunch) and leaves neither next_first nor a pre-staged tile behind, on every path
hipError_t train_bunches(bp_handle *h, int first, int nb);
// The pieces of a bunch, shared by bunch(), the CV / inference forward and the driver that cuts the step at the gradient
// exchange (bp_dp.hip):
hipError_t step_inputs(bp_handle *h, int first, const float **x0, const float **tg);   // stage / mask the bunch's rows; where they lie
// forward of weight layer l on M frames from the input rows x0 (bf16: converted at l == 1).  train: hidden outputs get the
// dropout mask and the output layer writes dEdX_L against tg; out (optional): the network outputs; alpha: keep-scale of the inputs
hipError_t step_forward(bp_handle *h, int l, int M, const float *x0, const float *tg, float *out, bool train, float alpha);
hipError_t step_dgrad(bp_handle *h, int l);                                             // dEdX_{l-1} from dEdX_l and the pre-update W_l
// weight + bias gradients of layers ls[0..n), ONE grouped launch where the kernel set allows it; fused: momentum update in the
// epilogue, else store into the flat gradient buffer.  done != null (store only): done[l] is a device counter every tile of
// layer l's segment bumps behind its stores (in-kernel hand-off); only legal when step_wgrads_count(h) says the launch really counts.
hipError_t step_wgrads(bp_handle *h, const int *ls, int n, const float *x0, bool fused, unsigned *const *done);
bool step_wgrads_count(const bp_handle *h);
unsigned step_wgrad_tiles(const bp_handle *h, int l);                                   // tiles of layer l in that launch
hipError_t step_shadow(bp_handle *h, int l);                                            // fp32 master W_l -> bf16 shadow (bf16 mode)
bool step_stages(const bp_handle *h);                                                   // the bunch's input rows go through the staged tile (window chunk | visible dropout)
// single launches on h->stream (bp_profile.hip: isolated kernel timing)
hipError_t launch_fwd(bp_handle *h, int l, int M, const float *y_prev, const float *targ, float *out, bool train, float alpha);
hipError_t launch_dgrad(bp_handle *h, int l, int M);
hipError_t launch_wgrad(bp_handle *h, int l, int M, const float *y_prev, bool fused);
hipError_t prof_mark(bp_handle *h, int kind);
// A window chunk written by kernels on h->stream (bp_wave.hip, bp_mix.hip): window_reserve sizes the staging set that is not
// current (rows_b bytes of raw frames, targ_b bytes of target frames, nat_b bytes of NAT rows, n_samples entries of each of the
// tables win_start | targ_frame | nat_row) and returns where they lie; window_adopt then makes it the resident window chunk with
// the bookkeeping of bp_upload_chunk_windows (with or without targets).
int window_reserve(bp_handle *h, size_t rows_b, size_t targ_b, size_t nat_b, size_t n_samples, float **rows, float **targ, float **nat,
                   int **tables);
int window_adopt(bp_handle *h, int n_samples, int fea_dim, int context, bool nat, bool with_targ);
// CV-semantics forward of samples [0, n) of the resident chunk into out_chunk (the partial last bunch included), no copy
int out_chunk_reserve(bp_handle *h, int n_frames);
int forward_resident(bp_handle *h, int n);                 // ... with the kernels of the handle's mode (bp_set_forward)
int forward_resident_as(bp_handle *h, int n, int mode);    // ... with those of `mode` (CV: always BP_FORWARD_DEFAULT; a stream: its own)
int outputs_to_host(bp_handle *h, int n);                  // rows [0, n) of out_chunk into host_out on h->stream, no synchronisation
int train_whole_chunk(bp_handle *h, int n);                // every whole bunch of the n resident rows; the remainder gets the reference's line

// ------------------------------------------------------------------ mixtures (bp_mix.hip)
void mix_free(bp_handle *h);                      // the corpus and the mixing buffers (bp_destroy)

// ------------------------------------------------------------------ streaming sessions (bp_stream.hip)
void stream_free_all(bp_handle *h);               // every open stream of the handle (bp_destroy)

// ------------------------------------------------------------------ data-parallel driver (bp_dp.hip)
int dp_check(bp_handle *h);                       // BP_OK, or the device-side timeout an exchange kernel raised
hipError_t dp_bunch(bp_handle *h, int first);
hipError_t dp_flush(bp_handle *h);
int dp_gather_deltas(bp_handle *h);
int dp_detach(bp_handle *h, bool gather);       // bp_dp_detach (gather: the sharded momentum state first) | bp_destroy (no gather)
bool dp_gathers_deltas(const bp_handle *h);       // attached with more than one rank: the momentum state is sharded
