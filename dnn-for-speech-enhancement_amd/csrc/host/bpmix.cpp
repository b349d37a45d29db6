// bpmix.cpp -- one training epoch on clean speech and noise mixed on the GPU, with bptrain's net and
// hyper-parameter keys, weight-file bytes and log layout, so that a Perl-style epoch loop can drive it like bptrain:
//
//   bpmix clean_list=clean.list noise_list=noise.list norm_file=mix.norm cv_clean_list=cv.list fea_dim=129 fea_context=11
//         targ_offset=5 numlayers=5 layersizes=1548,2048,2048,2048,129 bunchsize=256 lrate=... momentum=... weightcost=...
//         dropoutflag=1 visible_omit=0.1 hid_omit=0.2 traincache=100000 init_randem_seed=345 initwts_file=... outwts_file=...
//         log_file=... [snr_list=-5,0,5,10,15,20] [mix_per_clean=1] [target=lps|irm|ibm|lps+irm|lps+ibm] [lc_db=5]
//         [cv_noise_list=noise.list] [cv_seed=20261016] [mix_plan_out=plan.txt] [output_act=...] [compute=fp32|bf16] ...
//         [rir_list=rir.list] [reverb_target=reverberant|early] [early_ms=50] [cv_rir_list=rir.list]
//         [rir_rooms=N] [rir_room_lo=3,3,2.5] [rir_room_hi=10,8,4] [rir_t60=0.2,0.8] [rir_margin=0.5] [rir_dist=0.5,3] [rir_ms=400]
//         [rir_window=taps] [rir_rooms_out=rooms.txt] [cv_rir_rooms=N] [rate=8000] [nat=static|dynamic]
//         [aux_target=mfcc] [aux_rate=8000] [aux_mel=26] [aux_ceps=13] [aux_first=0] [aux_lifter=22] [aux_weight=1] [aux_norm_file=mfcc.norm]
//   bpmix clean_list=... noise_list=... fea_dim=129 norm_out=mix.norm [snr_list=...] [mix_per_clean=...] [init_randem_seed=...]
//   bpmix clean_list=... fea_dim=129 aux_target=mfcc aux_norm_out=mfcc.norm [aux_rate=...] [aux_mel=...] [aux_ceps=...] [aux_first=...] [aux_lifter=...]
//
// The plan of the epoch is bp_mix_plan(init_randem_seed, clean sentences, mix_per_clean, noise lengths, snr_list); it is cut into
// calls of at most traincache rows (frames + n_mix (context-1)) in plan order, and call k trains its frames in the order
// bp_mix_shuffle(init_randem_seed, k, frames of call k).  A driver that changes init_randem_seed per epoch gets new mixtures every
// epoch.  CV mixes cv_clean_list with cv_noise_list (default noise_list), one mixture per clean sentence, from cv_seed (fixed by
// default, so the CV error is comparable across epochs).  norm_out: per-bin mean and inverse std of the noisy LPS of one epoch's
// training mixtures, accumulated in double, in bpfeat's format; nothing is trained.  mix_plan_out: the drawn training plan, one
// `clean noise offset snr` line per mixture.  rir_list: one room impulse response per WAV, at the rate of the
// clean sentences; clean sentence c is paired with response bp_mix_reverb_pairs(init_randem_seed, ...)[c], the pairs become the
// derived entries n_clean + c of the corpus and the plan addresses entry n_clean + c in place of c.  reverb_target: what the net
// learns to produce, the reverberant sentence or its direct sound + early_ms of reflections.  CV: cv_rir_list (default rir_list),
// paired from cv_seed.  rir_rooms=N takes the place of rir_list: N simulated responses of rir_ms milliseconds
// at the rate of the clean sentences, their rooms drawn by bp_rir_rooms(init_randem_seed, N, the rir_* ranges) and made by
// bp_rir_image; rir_rooms_out lists the rooms, one `L src mic beta` line each; CV draws cv_rir_rooms (default N) from cv_seed.
// rate=R: every clean or noise WAV (training and CV) whose rate is not R is converted to R on the device as its
// list is loaded (bp_resample_waves: one call and one line on stdout per list and distinct rate; the float samples go on as they
// come), R is the rate of the corpus, and a response of rir_list must have it: an impulse response is not converted.
// aux_target=mfcc: the MFCC auxiliary target of multi-objective training.  The target row becomes
// [LPS | MFCC | mask]: target= must begin with lps, layersizes[last] is parts*fea_dim + aux_ceps, and the net wants
// output_linear_dims = fea_dim + aux_ceps (both logged).  aux_rate (default: rate=, else the rate of the clean sentences) places the
// aux_mel triangles between 0 and aux_rate / 2; aux_ceps coefficients from c0 (aux_first=1: from c1), HTK lifter aux_lifter (0:
// none).  aux_norm_file: mean and inverse std of the coefficients in the norm-file format, aux_ceps values each; aux_weight: the
// weight of the MFCC columns' squared error, folded as its square root into the scale.  aux_norm_out: those statistics of the clean
// sentences, one pass of bp_wave_mfcc, accumulated in double; nothing is trained and noise_list is not needed.
// Every key, list, WAV and drawn room is checked before the device is used (with rate=, before anything but the conversions).  Errors: message +
// exit(0); success: return 1 (reference convention).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <string>
#include <vector>

#include "../../../include/bp_c_api.h"
#include "corpus.h"
#include "keys.h"
#include "net_setup.h"
#include "rir_keys.h"
#include "wts_io.h"

namespace {

using namespace bp;
const char *const WHO = "bpmix";

struct Params {
    std::string clean_list, noise_list, cv_clean_list, cv_noise_list, norm_file, norm_out, mix_plan_out;
    std::string initwts_file, outwts_file, log_file, rir_list, cv_rir_list;
    int reverb_target = BP_REVERB_TARGET_REVERBERANT;
    int nat = BP_NAT_STATIC;                                 // nat=static|dynamic: the noise-aware block of the net's input (not read by norm_out)
    float early_ms = 50.0f;
    int fea_dim = 0, fea_context = 1, targ_offset = 0, dropoutflag = 0, traincache = 0, bunchsize = 0, numlayers = 0, gpu_used = 1;
    int layersizes[BP_MAXLAYER] = {0}, mix_per_clean = 1, target = BP_MIX_LPS, activation = 0, momentum_rule = 0, compute_dtype = 0;
    int output_act = 0, output_linear_dims = 0, output_loss = 0, device = 0, rate = 0;
    float momentum = 0, weightcost = 0, lrate = 0, visible_omit = 0, hid_omit = 0, lc_db = 5.0f;
    float wmin = -0.1f, wmax = 0.1f, bmin = -0.1f, bmax = 0.1f;
    unsigned long long seed = 0, cv_seed = 20261016ull, dropout_seed = 0;
    std::vector<float> snr = {-5, 0, 5, 10, 15, 20};
    RirKeys rir;
    int aux_target = 0, aux_rate = 0, aux_mel = 26, aux_ceps = 13, aux_first = 0;   // aux_target=mfcc (1): the MFCC auxiliary target
    float aux_lifter = 22.0f, aux_weight = 1.0f;
    std::string aux_norm_file, aux_norm_out;
    bool aux_keys = false;                                   // an aux_* key other than aux_target was given
};

Params parse(int argc, char **argv)
{
    Params P;
    const Key keys[] = {
        {"clean_list", K_STR, &P.clean_list}, {"noise_list", K_STR, &P.noise_list}, {"cv_clean_list", K_STR, &P.cv_clean_list},
        {"cv_noise_list", K_STR, &P.cv_noise_list}, {"norm_file", K_STR, &P.norm_file}, {"norm_out", K_STR, &P.norm_out},
        {"mix_plan_out", K_STR, &P.mix_plan_out}, {"initwts_file", K_STR, &P.initwts_file}, {"outwts_file", K_STR, &P.outwts_file},
        {"log_file", K_STR, &P.log_file}, {"rir_list", K_STR, &P.rir_list}, {"cv_rir_list", K_STR, &P.cv_rir_list},
        {"reverb_target", K_CHOICE, &P.reverb_target, BP_REVERB_TARGET_REVERBERANT, 0, "reverberant|early", "is not reverberant or early"},
        {"early_ms", K_FLOAT, &P.early_ms, 0, 1e6},
        {"fea_dim", K_INT, &P.fea_dim, 1, 1 << 20},
        {"fea_context", K_INT, &P.fea_context, 1, 1000},
        {"targ_offset", K_INT, &P.targ_offset, 0, 999},
        {"dropoutflag", K_INT, &P.dropoutflag, 0, 1},
        {"traincache", K_INT, &P.traincache, 1, BP_MAXCACHEFRAME},
        {"bunchsize", K_INT, &P.bunchsize, 1, 1 << 20},
        {"numlayers", K_INT, &P.numlayers, 2, BP_MAXLAYER - 1},
        {"gpu_used", K_INT, &P.gpu_used, 1, 1},                                      // (one GPU: mixing is single-device)
        {"device", K_INT, &P.device, 0, 1023},
        {"rate", K_INT, &P.rate, 1, (double)RATE_MAX},
        {"mix_per_clean", K_INT, &P.mix_per_clean, 1, 1 << 20},
        {"init_randem_seed", K_U64, &P.seed}, {"cv_seed", K_U64, &P.cv_seed}, {"seed", K_U64, &P.dropout_seed},
        {"lrate", K_FLOAT, &P.lrate}, {"momentum", K_FLOAT, &P.momentum}, {"weightcost", K_FLOAT, &P.weightcost},
        {"visible_omit", K_FLOAT, &P.visible_omit}, {"hid_omit", K_FLOAT, &P.hid_omit}, {"lc_db", K_FLOAT, &P.lc_db},
        {"init_randem_weight_min", K_FLOAT, &P.wmin}, {"init_randem_weight_max", K_FLOAT, &P.wmax},
        {"init_randem_bias_min", K_FLOAT, &P.bmin}, {"init_randem_bias_max", K_FLOAT, &P.bmax},
        {"layersizes", K_SIZES, P.layersizes, 0, BP_MAXLAYER - 1, nullptr, nullptr, &P.numlayers},
        {"snr_list", K_FLOATS, &P.snr},
        {"target", K_CHOICE, &P.target, BP_MIX_LPS, 0, "lps|irm|ibm|lps+irm|lps+ibm", "is not lps, irm, ibm, lps+irm or lps+ibm"},
        {"activation", K_CHOICE, &P.activation, 0, 0, "relu|sigmoid"},
        {"momentum_rule", K_CHOICE, &P.momentum_rule, 0, 0, "live|classic"},
        {"compute", K_CHOICE, &P.compute_dtype, 0, 0, "fp32|bf16"},
        {"output_act", K_CHOICE, &P.output_act, 0, 0, "linear|sigmoid"},
        {"output_linear_dims", K_INT, &P.output_linear_dims, 0, 1000000},
        {"output_loss", K_CHOICE, &P.output_loss, 0, 0, "xent|mse"},
        {"aux_target", K_CHOICE, &P.aux_target, 1, 0, "mfcc", "is not mfcc"},
    };
    const Key aux_keys[] = {
        {"aux_rate", K_INT, &P.aux_rate, 1, (double)RATE_MAX}, {"aux_mel", K_INT, &P.aux_mel, 2, 128}, {"aux_ceps", K_INT, &P.aux_ceps, 1, 128},
        {"aux_first", K_INT, &P.aux_first, 0, 1}, {"aux_lifter", K_FLOAT, &P.aux_lifter, 0, 1e6}, {"aux_weight", K_FLOAT, &P.aux_weight, 0, 1e12},
        {"aux_norm_file", K_STR, &P.aux_norm_file}, {"aux_norm_out", K_STR, &P.aux_norm_out},
    };
    for (int i = 1; i < argc; ++i) {
        const Arg a = split_arg(argv[i]);
        if (key_apply(aux_keys, WHO, a)) { P.aux_keys = true; continue; }
        if (key_apply(keys, WHO, a) || nat_key(a, WHO, nullptr, &P.nat)) continue;
        const int r = rir_key(P.rir, a.k, a.v);
        if (!r) fail("bpmix: unknown key " + a.k);
        if (r < 0) bad_value(WHO, a.k, a.v);
    }
    return P;
}

void one_rate(const std::string &what, const std::vector<int> &clean_rates)
{
    for (size_t k = 0; k < clean_rates.size(); ++k)
        if (clean_rates[k] != clean_rates[0])
            fail("bpmix: " + what + " needs clean sentences of one sample rate (sentence " + std::to_string(k) + " has " +
                 std::to_string(clean_rates[k]) + " Hz, sentence 0 " + std::to_string(clean_rates[0]) + " Hz)");
}
// The impulse responses of a rir_list, checked against the rate of the clean sentences (on: the list was given); else
// n_rooms > 0: rooms drawn from the seed (checked here, made on the device by set_reverb)
Reverb read_reverb(const Params &P, const std::string &what, const std::string &list, int n_rooms, unsigned long long seed,
                   const std::vector<int> &clean_rates)
{
    Reverb r;
    if (list.empty() && n_rooms > 0) {
        one_rate("rir_rooms", clean_rates);
        const std::string err = rir_draw(P.rir, seed, n_rooms, clean_rates[0], r.rooms, r.len);
        if (!err.empty()) fail("bpmix: " + err);
        r.on = true; r.target = P.reverb_target; r.rate = clean_rates[0];
        r.early_taps = early_taps(P.early_ms, clean_rates[0]);
        return r;
    }
    if (list.empty()) return r;
    std::vector<int> rates;
    const auto w = read_wav_list(WHO, what, list, &rates);
    one_rate(what, clean_rates);
    for (size_t k = 0; k < w.size(); ++k) {
        if (P.rate && rates[k] != P.rate)
            fail("bpmix: " + what + ": response " + std::to_string(k) + " has " + std::to_string(rates[k]) + " Hz and rate=" + std::to_string(P.rate) +
                 " does not convert impulse responses (resampling one also rescales it)");
        if (rates[k] != clean_rates[0])
            fail("bpmix: " + what + ": response " + std::to_string(k) + " has " + std::to_string(rates[k]) + " Hz, the clean sentences " +
                 std::to_string(clean_rates[0]) + " Hz");
        if (w[k].size() > (size_t)BP_MIX_RIR_MAX_TAPS)
            fail("bpmix: " + what + ": response " + std::to_string(k) + " has more than " + std::to_string(BP_MIX_RIR_MAX_TAPS) + " taps");
        for (float v : w[k])
            if (!std::isfinite(v)) fail("bpmix: " + what + ": response " + std::to_string(k) + " has a tap that is not finite");
        r.pcm.insert(r.pcm.end(), w[k].begin(), w[k].end());
        r.len.push_back((int)w[k].size());
    }
    r.on = true; r.target = P.reverb_target;
    r.early_taps = early_taps(P.early_ms, clean_rates[0]);
    return r;
}

// aux_target=mfcc: the parameters of the keys at the corpus' rate, checked against fea_dim on the host (no mean / scale yet)
bp_mel_params aux_params(const Params &P, const std::vector<int> &clean_rates)
{
    int rate = P.aux_rate ? P.aux_rate : P.rate;
    if (!rate) { one_rate("aux_target", clean_rates); rate = clean_rates[0]; }
    bp_mel_params mp;
    check(bp_mel_defaults(rate, &mp));
    mp.n_mel = P.aux_mel; mp.n_ceps = P.aux_ceps; mp.first_coef = P.aux_first; mp.lifter = P.aux_lifter;
    if (bp_mel_filters(P.fea_dim, &mp, nullptr, nullptr, nullptr) != 0) fail(std::string("bpmix: aux_target: ") + bp_last_error());
    return mp;
}

// aux_norm_out: mean and inverse std of the MFCC of the clean sentences (the norm-file format, aux_ceps values), bp_wave_mfcc in
// calls of at most 2^24 samples
int aux_norm_pass(const Params &P, const Corpus &clean, bp_mel_params mp)
{
    const int D = P.fea_dim, hop = D - 1, nc = mp.n_ceps, ns = (int)clean.len.size();
    FILE *fn = fopen(P.aux_norm_out.c_str(), "wt");
    if (!fn) fail("can not open norm file: " + P.aux_norm_out);
    std::vector<double> sum(nc, 0.0), sq(nc, 0.0);
    std::vector<float> cc;
    std::vector<int> lens;
    size_t total = 0, at = 0;
    for (int s0 = 0; s0 < ns;) {
        int s1 = s0;
        size_t n = 0, T = 0;
        lens.clear();
        while (s1 < ns && (s1 == s0 || n + (size_t)clean.len[s1] <= ((size_t)1 << 24))) {
            lens.push_back((int)clean.len[s1]);
            n += (size_t)clean.len[s1]; T += ((size_t)clean.len[s1] - 1) / hop + 2;
            ++s1;
        }
        cc.resize(T * nc);
        check(bp_wave_mfcc(P.device, D, &mp, s1 - s0, lens.data(), clean.pcm.data() + at, nullptr, nullptr, cc.data()));
        for (size_t f = 0; f < T; ++f)
            for (int r = 0; r < nc; ++r) { const double v = cc[f * nc + r]; sum[r] += v; sq[r] += v * v; }
        total += T; at += n; s0 = s1;
    }
    write_norm(fn, sum, sq, total);
    printf("bpmix: MFCC norm file of %zu clean frames of %d sentences -> %s\n", total, ns, P.aux_norm_out.c_str());
    return 1;
}

// norm_out: mean and inverse std of the noisy LPS of the epoch's training mixtures (bpfeat's format), on a one-layer handle
int norm_pass(const Params &P, const Corpus &clean, const Corpus &noise, std::vector<bp_mixture> plan, const Reverb &rv)
{
    const int D = P.fea_dim, hop = D - 1, cap = P.traincache ? P.traincache : BP_MAXCACHEFRAME;
    std::vector<int> frames;
    const auto calls = cut(WHO, plan, clean, hop, 1, cap, &frames);
    FILE *fn = fopen(P.norm_out.c_str(), "wt");
    if (!fn) fail("can not open norm file: " + P.norm_out);
    const int ls[2] = {D, D};
    bp_config cfg = net_config(2, ls, 256, cap, P.device);
    Weights wts(2, ls);
    std::vector<float> mean(D, 0.f), istd(D, 1.f);
    bp_handle *h = nullptr;
    check(bp_create(&cfg, wts.weights, wts.bias, &h));
    const bp_mix_corpus mc = describe(D, 1, 0, BP_MIX_LPS, P.lc_db, mean.data(), istd.data(), clean, noise);
    check(bp_set_mix_corpus(h, &mc));
    if (rv.on) set_reverb(h, P.rir, P.device, rv, P.seed, (int)clean.len.size());
    address_reverberant(plan, rv, (int)clean.len.size());
    std::vector<double> sum(D, 0.0), sq(D, 0.0);
    size_t total = 0;
    std::vector<float> lps;
    for (size_t k = 0; k < calls.size(); ++k) {
        const int n = calls[k].second - calls[k].first;
        lps.resize((size_t)frames[k] * D);
        check(bp_mix_features(h, n, plan.data() + calls[k].first, nullptr, lps.data(), nullptr, nullptr, nullptr));
        for (int f = 0; f < frames[k]; ++f)
            for (int j = 0; j < D; ++j) { const double v = lps[(size_t)f * D + j]; sum[j] += v; sq[j] += v * v; }
        total += (size_t)frames[k];
    }
    bp_destroy(h);
    write_norm(fn, sum, sq, total);
    printf("bpmix: norm file of %zu noisy frames of %zu mixtures -> %s\n", total, plan.size(), P.norm_out.c_str());
    return 1;
}

}  // namespace

int main(int argc, char **argv)
{
    const double t_start = (double)time(NULL);
    const Params P = parse(argc, argv);
    const int D = P.fea_dim;
    check_fea_dim(WHO, D);
    if (P.snr.empty()) fail("bpmix: snr_list is empty");
    const int hop = D - 1;
    // every list and WAV is read and checked before the device is used
    std::vector<int> clean_rates, cv_rates;
    const Corpus clean = flatten(read_wav_list(WHO, "clean_list", P.clean_list, &clean_rates, nullptr, P.rate, P.device));
    if (P.aux_keys && !P.aux_target) fail("bpmix: the aux_* keys need aux_target=mfcc");
    bp_mel_params mp;
    memset(&mp, 0, sizeof(mp));
    if (P.aux_target) {
        mp = aux_params(P, clean_rates);
        if (!P.aux_norm_out.empty()) return aux_norm_pass(P, clean, mp);
    }
    const Corpus noise = flatten(read_wav_list(WHO, "noise_list", P.noise_list, nullptr, nullptr, P.rate, P.device));
    check_noise(WHO, noise);
    std::vector<bp_mixture> plan = make_plan(P.seed, (int)clean.len.size(), P.mix_per_clean, noise, P.snr);
    check_rir_keys(WHO, P.rir, P.rir_list, P.cv_rir_list, "");
    const Reverb rv = read_reverb(P, "rir_list", P.rir_list, P.rir.rooms, P.seed, clean_rates);
    if (!P.rir.rooms_out.empty()) {
        const std::string err = rir_write_rooms(P.rir.rooms_out, rv.rooms);
        if (!err.empty()) fail(err);
    }
    if (!P.norm_out.empty()) return norm_pass(P, clean, noise, plan, rv);

    const int L = P.numlayers, ctx = P.fea_context, toff = P.targ_offset;
    if (L < 2 || P.layersizes[L - 1] < 1) fail("bpmix: numlayers / layersizes: need 2.." + std::to_string(BP_MAXLAYER - 1) + " layer sizes");
    if (P.outwts_file.empty() || P.log_file.empty() || P.norm_file.empty()) fail("bpmix: need norm_file, outwts_file and log_file");
    if (P.traincache < 1 || P.bunchsize < 1) fail("bpmix: need traincache and bunchsize");
    if (toff >= ctx) fail("bpmix: targ_offset must be below fea_context");
    const int parts = P.target == BP_MIX_LPS_IRM || P.target == BP_MIX_LPS_IBM ? 2 : 1;
    if (P.aux_target) {
        if (P.target != BP_MIX_LPS && parts != 2) fail("bpmix: aux_target=mfcc needs a target that begins with lps (lps, lps+irm or lps+ibm)");
        if (P.layersizes[L - 1] != parts * D + mp.n_ceps)
            fail("bpmix: layersizes[last] must be " + std::to_string(parts * D + mp.n_ceps) + " for this target with aux_target=mfcc (aux_ceps columns behind the LPS)");
    } else if (P.layersizes[L - 1] != parts * D) fail("bpmix: layersizes[last] must be " + std::to_string(parts * D) + " for this target");
    if (P.layersizes[0] != ctx * D && P.layersizes[0] != (ctx + 1) * D) fail("bpmix: layersizes[0] must be fea_context*fea_dim (+ fea_dim with NAT)");
    const Corpus cv_clean = flatten(read_wav_list(WHO, "cv_clean_list", P.cv_clean_list, &cv_rates, nullptr, P.rate, P.device));
    const Corpus cv_noise = P.cv_noise_list.empty() ? noise : flatten(read_wav_list(WHO, "cv_noise_list", P.cv_noise_list, nullptr, nullptr, P.rate, P.device));
    std::vector<bp_mixture> cv_plan = make_plan(P.cv_seed, (int)cv_clean.len.size(), 1, cv_noise, P.snr);
    const Reverb cv_rv = read_reverb(P, P.cv_rir_list.empty() ? "rir_list" : "cv_rir_list", P.cv_rir_list.empty() ? P.rir_list : P.cv_rir_list,
                                     P.rir.rooms ? (P.rir.cv_rooms ? P.rir.cv_rooms : P.rir.rooms) : 0, P.cv_seed, cv_rates);
    std::vector<int> frames, cv_frames;
    const auto calls = cut(WHO, plan, clean, hop, ctx, P.traincache, &frames);
    const auto cv_calls = cut(WHO, cv_plan, cv_clean, hop, ctx, P.traincache, &cv_frames);
    address_reverberant(plan, rv, (int)clean.len.size());
    address_reverberant(cv_plan, cv_rv, (int)cv_clean.len.size());
    std::vector<float> mean, istd;
    read_norm(P.norm_file, D, mean, istd);
    std::vector<float> aux_mean(mp.n_ceps, 0.f), aux_scale(mp.n_ceps, 1.f);
    if (P.aux_target) {
        if (!P.aux_norm_file.empty()) read_norm(P.aux_norm_file, mp.n_ceps, aux_mean, aux_scale);
        for (float &v : aux_scale) v = (float)((double)v * sqrt((double)P.aux_weight));   // a weight on the squared error is its root on the target
        mp.mean = aux_mean.data(); mp.scale = aux_scale.data();
    }

    FILE *log = fopen(P.log_file.c_str(), "wt");
    if (!log) fail("can not open output log file: " + P.log_file);
    FILE *fp_out = fopen(P.outwts_file.c_str(), "wb");
    if (!fp_out) { fprintf(log, "can not open output weights file: %s\n", P.outwts_file.c_str()); exit(0); }
    if (!P.mix_plan_out.empty()) {
        FILE *fo = fopen(P.mix_plan_out.c_str(), "wt");
        if (!fo) { fprintf(log, "can not open plan file: %s\n", P.mix_plan_out.c_str()); exit(0); }
        for (const bp_mixture &m : plan) fprintf(fo, "%d %d %lld %.9g\n", m.clean, m.noise, (long long)m.offset, m.snr_db);
        fclose(fo);
    }
    fprintf(log, "parameters input:\n");
    fprintf(log, "clean_list:           %s\n", P.clean_list.c_str());
    fprintf(log, "noise_list:           %s\n", P.noise_list.c_str());
    fprintf(log, "cv_clean_list:        %s\n", P.cv_clean_list.c_str());
    fprintf(log, "norm_file:            %s\n", P.norm_file.c_str());
    fprintf(log, "outwts_file:          %s\n", P.outwts_file.c_str());
    fprintf(log, "log_file:\t\t          %s\n", P.log_file.c_str());
    fprintf(log, "initwts_file:         %s\n", P.initwts_file.c_str());
    fprintf(log, "fea_dim:\t\t          %d\n", D);
    fprintf(log, "fea_context:\t\t      %d\n", ctx);
    fprintf(log, "bunchsize:\t\t        %d\n", P.bunchsize);
    fprintf(log, "train_cache:\t\t      %d\n", P.traincache);
    fprintf(log, "init_randem_seed:\t\t  %llu\n", P.seed);
    fprintf(log, "targ_offset:\t\t      %d\n", toff);
    fprintf(log, "dropoutflag:\t\t      %d\n", P.dropoutflag);
    fprintf(log, "momentum:\t\t                %f\n", P.momentum);
    fprintf(log, "weightcost:\t\t              %f\n", P.weightcost);
    fprintf(log, "learnrate:\t\t              %f\n", P.lrate);
    fprintf(log, "visible_omit:\t\t      %f\n", P.visible_omit);
    fprintf(log, "hid_omit:\t\t      %f\n", P.hid_omit);
    fprintf(log, "mix_per_clean:\t\t    %d\n", P.mix_per_clean);
    fprintf(log, "lc_db:\t\t            %f\n", P.lc_db);
    fprintf(log, "layersizes:\t\t              ");
    for (int j = 0; j < L; ++j) fprintf(log, "%d,", P.layersizes[j]);
    fprintf(log, "\nPlease check...\n");

    Weights wts(L, P.layersizes);
    srand48((long)P.seed);
    if (P.initwts_file.empty()) {
        fprintf(log, "Getting Randemed initial weights...\n");
        random_weights(L, P.layersizes, wts.weights, wts.bias, P.wmin, P.wmax, P.bmin, P.bmax);
        fprintf(log, "Randemed initial weights getted.\n");
    } else {
        const std::string err = load_weights(P.initwts_file, L, P.layersizes, wts, log);
        if (!err.empty()) { fprintf(log, "%s\n", err.c_str()); exit(0); }
        fprintf(log, "Init weight file loaded.\n");
    }
    fflush(log);

    bp_config cfg = net_config(L, P.layersizes, P.bunchsize, P.traincache, P.device);
    cfg.lrate = P.lrate; cfg.momentum = P.momentum; cfg.weightcost = P.weightcost;
    cfg.dropoutflag = P.dropoutflag; cfg.visible_omit = P.visible_omit; cfg.hid_omit = P.hid_omit;
    cfg.activation = P.activation; cfg.momentum_rule = P.momentum_rule; cfg.seed = P.dropout_seed; cfg.compute_dtype = P.compute_dtype;
    bp_handle *h = create_net(cfg, wts, P.output_act, P.output_linear_dims, P.output_loss);
    printf("Created net with %d layers, bunchsize %d.\n", L, P.bunchsize);
    set_nat(WHO, h, P.nat, ctx, D, P.layersizes);
    if (P.aux_target) {
        check(bp_set_mix_aux(h, &mp));
        fprintf(log, "Auxiliary target: mfcc, %d filters up to %d Hz, %d coefficients from c%d, lifter %g, weight %g: target columns [%d, %d).\n",
                mp.n_mel, mp.sample_rate / 2, mp.n_ceps, mp.first_coef, mp.lifter, P.aux_weight, D, D + mp.n_ceps);
        fprintf(log, "Auxiliary target: the net's linear prefix is output_linear_dims=%d (LPS and MFCC columns), given %d.\n", D + mp.n_ceps,
                P.output_linear_dims);
    }
    const bp_mix_corpus mc = describe(D, ctx, toff, P.target, P.lc_db, mean.data(), istd.data(), clean, noise);
    check(bp_set_mix_corpus(h, &mc));
    if (rv.on) {
        set_reverb(h, P.rir, P.device, rv, P.seed, (int)clean.len.size());
        fprintf(log, "Reverberation: %zu %simpulse responses, target %s, %d early taps.\n", rv.len.size(), rv.rooms.empty() ? "" : "simulated ",
                rv.target == BP_REVERB_TARGET_EARLY ? "early" : "reverberant", rv.early_taps);
    }
    fprintf(log, "Corpus loaded: %zu clean sentences, %zu noise recordings, %zu mixtures in %zu chunks.\n", clean.len.size(),
            noise.len.size(), plan.size(), calls.size());
    struct timespec ts0, ts1;
    clock_gettime(CLOCK_MONOTONIC, &ts0);
    long total = 0;
    std::vector<int> order;
    for (size_t k = 0; k < calls.size(); ++k) {
        fprintf(log, "Starting chunk %d of %d containing %d samples.\n", (int)k + 1, (int)calls.size(), frames[k]);
        fflush(log);
        order.resize(frames[k]);
        check(bp_mix_shuffle(P.seed, (uint32_t)k, frames[k], order.data()));
        check(bp_set_hyper(h, P.lrate, P.momentum, P.weightcost, P.dropoutflag, P.visible_omit, P.hid_omit));
        check(bp_train_mix(h, calls[k].second - calls[k].first, plan.data() + calls[k].first, order.data()));
        total += frames[k];
    }
    printf("begin to write weights\n");
    check(bp_get_weights(h, wts.weights, wts.bias));
    clock_gettime(CLOCK_MONOTONIC, &ts1);
    {
        const double dt = (double)(ts1.tv_sec - ts0.tv_sec) + 1e-9 * (double)(ts1.tv_nsec - ts0.tv_nsec);
        fprintf(log, "Training pass: %ld samples in %.3f s (%.0f frames/s, mixing + GPU).\n", total, dt, dt > 0 ? total / dt : 0.0);
    }
    fprintf(log, "Saving weights to file...\n");
    write_weights(fp_out, L, P.layersizes, wts.weights, wts.bias);
    fclose(fp_out);
    fprintf(log, "Saving over.\n");
    printf("finish to write weights\n\n");

    printf("begin to CV\n");
    fprintf(log, "Starting CV.\n");
    const bp_mix_corpus cvc = describe(D, ctx, toff, P.target, P.lc_db, mean.data(), istd.data(), cv_clean, cv_noise);
    check(bp_set_mix_corpus(h, &cvc));
    if (cv_rv.on) set_reverb(h, P.rir, P.device, cv_rv, P.cv_seed, (int)cv_clean.len.size());
    fprintf(log, "Get cv chunk info over: CV mixtures have %d chunks.\n", (int)cv_calls.size());
    float squared_err = 0.0f;
    long cv_total = 0;
    for (size_t k = 0; k < cv_calls.size(); ++k) {
        float e = 0.0f;
        printf("cur_chunk_samples=%d\n", cv_frames[k]);
        check(bp_set_hyper(h, P.lrate, P.momentum, P.weightcost, P.dropoutflag, P.visible_omit, P.hid_omit));
        check(bp_cv_mix(h, cv_calls[k].second - cv_calls[k].first, cv_plan.data() + cv_calls[k].first, &e));
        squared_err += e;
        cv_total += cv_frames[k];
    }
    const float cvacc = squared_err / cv_total;                          // (bptrain: BPtrain.cc:84)
    fprintf(log, "CV over. squared error: %f\n", cvacc);
    fprintf(log, "Total cost time: %.1f s.\n", (double)time(NULL) - t_start);
    printf("all finish!\n");
    bp_destroy(h);
    fclose(log);
    return 1;
}
