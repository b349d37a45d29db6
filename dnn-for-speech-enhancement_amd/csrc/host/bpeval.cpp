// bpeval.cpp -- objective scores of enhanced speech on the MI355X: segmental SNR, log-spectral distortion and
// STOI, through bp_eval_mix (a test set mixed on the GPU and enhanced with a trained net) or bp_score_waves (pairs of WAVs); with
// scores=extended|full|all the further columns of COLUMNS behind them, through the _ext calls.
//
//   bpeval clean_list=test_clean.list noise_list=test_noise.list norm_file=x.norm initwts_file=mlp.N.wts fea_dim=129 fea_context=11
//          targ_offset=5 layersizes=1548,2048,2048,2048,129 [snr_list=-5,0,5,10,15,20] [mix_per_clean=1] [init_randem_seed=0]
//          [wave_target=lps|mask] [out_col=0] [traincache=102400] [bunchsize=1024] [dropoutflag=1 visible_omit=0.1 hid_omit=0.2]
//          [activation=relu|sigmoid] [compute=fp32|bf16] [output_act=... output_linear_dims=... output_loss=...] [device=0]
//          [scores_out=scores.txt] [baseline=logmmse] [rir_list=rir.list] [reverb_target=reverberant|early] [early_ms=50]
//          [scores=basic|extended|full|all] [rate=16000] [lm_noise=vad|spp] [nat=static|dynamic]
//          [post_gv=gv.norm] [post_mask_col=129 [post_mask_lo=0.5] [post_mask_hi=0.5] [post_mask_weight=1]]
//          [gv_out=gv.norm [gv_mode=indep|dep]]
//   bpeval pairs_list=<"ref.wav est.wav" per line> fea_dim=129 [device=0] [scores_out=scores.txt] [scores=basic|extended|full|all] [rate=16000]
//
// rate=R (either mode): every clean, noise or pair WAV whose rate is not R is converted to R on the device as it is
// loaded (bp_resample_waves: one call and one line on stdout per list and distinct rate), and R is the rate handed to the scores;
// a response of rir_list must have it: an impulse response is not converted.
// Test-set mode: the plan is bp_mix_plan(init_randem_seed, clean sentences, mix_per_clean, noise lengths, snr_list), cut into calls
// of at most traincache rows (frames + n_mix (context-1)) in plan order, as bpmix cuts it; every WAV must have the same rate (or rate=).
// stdout: one line per SNR (ascending) and one "all:" line, noisy -> enhanced; means skip NaN, and the count of NaN scores of the
// line is printed.  scores_out: one line per mixture in plan order, `clean noise offset snr ssnr_noisy ssnr_enh lsd_noisy lsd_enh
// stoi_noisy stoi_enh` (%.9g: the floats round-trip); pairs mode: `ref est ssnr lsd stoi` per pair.  Every key, list and WAV is
// checked before the device is used.  baseline=logmmse (test-set mode only) scores the classic log-MMSE enhancer on the same
// mixtures beside the net (bp_eval_mix_logmmse): after every stdout line a second one with `logmmse:` in place of
// the net's figures (noisy -> logmmse), and three more columns `ssnr_lm lsd_lm stoi_lm` at the end of every scores_out line.
// lm_noise=spp (only with baseline=logmmse; default vad: the output above, byte for byte) gives the baseline the MMSE-SPP noise tracker
// (bp_eval_mix_logmmse_nt).
// scores=extended|full|all (default basic: the output above, byte for byte): the columns of COLUMNS below that the value has, in its
// order.  Every stdout line gains `, NAME a -> b` with the column's unit per added column before the undefined count, which then
// counts the NaN of all columns; scores_out lines gain `x_noisy x_enh` per added column behind stoi_enh, the baseline's `x_lm` each
// behind its three, and pairs mode `x` each behind stoi.  scores=all: the rate must be 8 kHz or more.
// rir_list: one room impulse response per WAV, at the rate of the others; clean sentence c is paired with response
// bp_mix_reverb_pairs(init_randem_seed, ...)[c], the plan addresses the derived entry n_clean + c in place of c (so scores_out
// lists it), the mixtures are reverberant and the scores are taken against reverb_target: the reverberant sentence or its direct
// sound + early_ms of reflections.  rir_rooms=N with rir_room_lo / rir_room_hi / rir_t60 / rir_margin / rir_dist / rir_ms / rir_window /
// rir_rooms_out (bpmix's keys, its defaults) takes the place of rir_list: N simulated responses, their rooms drawn
// by bp_rir_rooms(init_randem_seed, N, ...) and made by bp_rir_image at the rate of the others.
// post_gv / post_mask_* (test-set mode, wave_target=lps; without them the output above, byte for byte): the net's
// LPS estimate is post-processed before resynthesis (bp_set_post) -- GV equalisation with the factors of the file, and the mask gate
// on the columns from post_mask_col on.  gv_out=FILE makes that file and scores nothing, as bpmix norm_out= trains nothing:
// bp_gv_mix over the plan in the same cuts, the sums added in call order, bp_gv_factors (gv_mode, default indep), centre then scale
// in norm-file format, and one line on stdout.
// Errors: message + exit(0); success: return 1 (reference convention).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../../include/bp_c_api.h"
#include "corpus.h"
#include "keys.h"
#include "net_setup.h"
#include "rir_keys.h"

namespace {

using namespace bp;
const char *const WHO = "bpeval";

struct Params {
    std::string clean_list, noise_list, pairs_list, norm_file, initwts_file, scores_out, rir_list;
    int reverb_target = BP_REVERB_TARGET_REVERBERANT;
    float early_ms = 50.0f;
    int fea_dim = 0, fea_context = 1, targ_offset = 0, dropoutflag = 0, traincache = 102400, bunchsize = 1024, numlayers = 0;
    int layersizes[BP_MAXLAYER] = {0}, mix_per_clean = 1, activation = 0, compute_dtype = 0, device = 0;
    int output_act = 0, output_linear_dims = 0, output_loss = 0, wave_target = BP_WAVE_LPS, out_col = 0, rate = 0;
    float visible_omit = 0, hid_omit = 0;
    unsigned long long seed = 0;
    std::vector<float> snr = {-5, 0, 5, 10, 15, 20};
    bool net_keys = false;                                   // a key of test-set mode was given
    int baseline = 0;                                        // baseline=logmmse
    int lm_noise = BP_NOISE_VAD;                             // lm_noise=vad|spp
    bool lm_noise_given = false;
    int nat = BP_NAT_STATIC;                                 // nat=static|dynamic: the noise-aware block of the net's input
    int ext = 0;                                             // scores=basic|extended|full|all: 0, 1, 2, 3 -> three, five, seven, nine score columns
    RirKeys rir;                                             // rir_rooms=N ...: simulated responses in place of rir_list
    PostKeys post;                                           // post_gv / post_mask_*: post-processing of the LPS estimate
    std::string gv_out;                                      // gv_out=FILE: the GV factors of the net on this test set, nothing scored
    int gv_mode = BP_GV_INDEP;
    bool gv_mode_given = false;
};

Params parse(int argc, char **argv)
{
    Params P;
    const Key both[] = {                                     // the keys of pairs mode, which test-set mode takes too
        {"pairs_list", K_STR, &P.pairs_list}, {"scores_out", K_STR, &P.scores_out},
        {"fea_dim", K_INT, &P.fea_dim, 1, 1 << 20},
        {"device", K_INT, &P.device, 0, 1023},
        {"scores", K_CHOICE, &P.ext, 0, 0, "basic|extended|full|all"},
        {"rate", K_INT, &P.rate, 1, (double)RATE_MAX},
    };
    const Key keys[] = {
        {"clean_list", K_STR, &P.clean_list}, {"noise_list", K_STR, &P.noise_list}, {"norm_file", K_STR, &P.norm_file},
        {"initwts_file", K_STR, &P.initwts_file}, {"rir_list", K_STR, &P.rir_list},
        {"reverb_target", K_CHOICE, &P.reverb_target, BP_REVERB_TARGET_REVERBERANT, 0, "reverberant|early", "is not reverberant or early"},
        {"early_ms", K_FLOAT, &P.early_ms, 0, 1e6},
        {"fea_context", K_INT, &P.fea_context, 1, 1000},
        {"targ_offset", K_INT, &P.targ_offset, 0, 999},
        {"dropoutflag", K_INT, &P.dropoutflag, 0, 1},
        {"traincache", K_INT, &P.traincache, 1, BP_MAXCACHEFRAME},
        {"bunchsize", K_INT, &P.bunchsize, 1, 1 << 20},
        {"mix_per_clean", K_INT, &P.mix_per_clean, 1, 1 << 20},
        {"out_col", K_INT, &P.out_col, 0, 1 << 20},
        {"output_linear_dims", K_INT, &P.output_linear_dims, 0, 1000000},
        {"visible_omit", K_FLOAT, &P.visible_omit}, {"hid_omit", K_FLOAT, &P.hid_omit},
        {"init_randem_seed", K_U64, &P.seed},
        {"layersizes", K_SIZES, P.layersizes, 0, BP_MAXLAYER - 1, nullptr, nullptr, &P.numlayers},
        {"snr_list", K_FLOATS, &P.snr},
        {"baseline", K_CHOICE, &P.baseline, 1, 0, "logmmse"},
        {"wave_target", K_CHOICE, &P.wave_target, BP_WAVE_LPS, 0, "lps|mask"},
        {"activation", K_CHOICE, &P.activation, 0, 0, "relu|sigmoid"},
        {"compute", K_CHOICE, &P.compute_dtype, 0, 0, "fp32|bf16"},
        {"output_act", K_CHOICE, &P.output_act, 0, 0, "linear|sigmoid"},
        {"output_loss", K_CHOICE, &P.output_loss, 0, 0, "xent|mse"},
        {"gv_out", K_STR, &P.gv_out},
    };
    const Key gv_mode[] = {{"gv_mode", K_CHOICE, &P.gv_mode, BP_GV_INDEP, 0, "indep|dep"}};
    for (int i = 1; i < argc; ++i) {
        const Arg a = split_arg(argv[i]);
        if (key_apply(both, WHO, a)) continue;
        if (lm_noise_key(a, WHO, nullptr, &P.lm_noise)) P.lm_noise_given = true;
        else if (nat_key(a, WHO, nullptr, &P.nat) || post_key(a, WHO, false, &P.post)) {}
        else if (key_apply(gv_mode, WHO, a)) P.gv_mode_given = true;
        else if (!key_apply(keys, WHO, a)) {
            const int r = rir_key(P.rir, a.k, a.v);
            if (!r) fail("bpeval: unknown key " + a.k);
            if (r < 0) bad_value(WHO, a.k, a.v);
        }
        P.net_keys = true;
    }
    if (P.lm_noise_given && !P.baseline && P.pairs_list.empty()) fail("bpeval: lm_noise needs baseline=logmmse");
    if (P.gv_mode_given && P.gv_out.empty() && P.pairs_list.empty()) fail("bpeval: gv_mode needs gv_out");
    return P;
}

void check_rate(int fs)
{
    int a = 10000, b = fs;
    while (b) { const int t = a % b; a = b; b = t; }
    if (fs <= 0 || 10000 / a > 32 || fs / a > 32)
        fail("bpeval: " + std::to_string(fs) + " Hz is not a scoring rate (8, 10, 12, 16, 20, 24, 32, 48 kHz)");
}

// mean over the finite values; NaN count.  Slot k < BP_SCORE_ALL_N: column k of the noisy side, BP_SCORE_ALL_N + k: of the enhanced
// side; ns: the columns the rows have
struct Acc { double sum[BP_SCORE_ALL_N * 2] = {0}; int cnt[BP_SCORE_ALL_N * 2] = {0}, n = 0, nan = 0; };
// The score columns in row order (BP_SCORE_*): name and unit on stdout, digits there, and the narrowest scores= value
// (0 .. 3: basic, extended, full, all) whose rows have the column
const struct { const char *name, *unit; int digits, ext; } COLUMNS[BP_SCORE_ALL_N] = {
    {"SSNR", " dB", 3, 0}, {"LSD", " dB", 3, 0}, {"STOI", "", 4, 0}, {"ESTOI", "", 4, 1}, {"SI-SDR", " dB", 3, 1},
    {"LLR", "", 4, 2}, {"CD", " dB", 3, 2}, {"fwSegSNR", " dB", 3, 3}, {"WSS", "", 3, 3},
};
int n_columns(int ext) { int ns = 0; while (ns < BP_SCORE_ALL_N && COLUMNS[ns].ext <= ext) ++ns; return ns; }
// the scores of one scores_out line: per column ` a` or, with b, ` a b`
void put_scores(FILE *fo, int ns, const float *a, const float *b = nullptr)
{
    for (int k = 0; k < ns; ++k) {
        fprintf(fo, " %.9g", a[k]);
        if (b) fprintf(fo, " %.9g", b[k]);
    }
}
void add(Acc &a, int ns, const float *noisy, const float *enh)
{
    ++a.n;
    for (int side = 0; side < 2; ++side)
        for (int k = 0; k < ns; ++k) {
            const float v = side ? enh[k] : noisy[k];
            if (std::isnan(v)) { ++a.nan; continue; }
            a.sum[side * BP_SCORE_ALL_N + k] += v; ++a.cnt[side * BP_SCORE_ALL_N + k];
        }
}
double avg(const Acc &a, int k) { return a.cnt[k] ? a.sum[k] / a.cnt[k] : NAN; }
// the means of one stdout line: per column `, <who>NAME a` or, with both sides, `, <who>NAME a -> b`, then the unit (who: before
// the first column alone)
void put_means(int ns, const Acc &a, bool both, const char *who = "")
{
    for (int k = 0; k < ns; ++k) {
        const int d = COLUMNS[k].digits;
        printf(", %s%s %.*f", k ? "" : who, COLUMNS[k].name, d, avg(a, k));
        if (both) printf(" -> %.*f", d, avg(a, BP_SCORE_ALL_N + k));
        printf("%s", COLUMNS[k].unit);
    }
}

int pairs_mode(const Params &P)
{
    if (P.net_keys) fail("bpeval: pairs_list takes only fea_dim, device and scores_out");   // (baseline= counts as a key of test-set mode)
    std::vector<std::string> refs, ests;
    read_pairs(WHO, "pairs_list", "pairs list", "a reference and an estimate", P.pairs_list, refs, ests);
    std::vector<float> r, e;
    std::vector<int> lens;
    int rate = 0;
    std::vector<std::vector<float>> both;                    // rate=: reference and estimate of every pair, to be converted together
    std::vector<int> both_rates;
    for (size_t i = 0; i < refs.size(); ++i) {
        int rr = 0, re = 0;
        const std::vector<float> a = read_one(WHO, refs[i], &rr), b = read_one(WHO, ests[i], &re);
        if (rr != re) fail("bpeval: " + refs[i] + " and " + ests[i] + " differ in sample rate");
        if (a.size() != b.size()) fail("bpeval: " + refs[i] + " and " + ests[i] + " differ in length");
        if (P.rate) check_convertible(WHO, refs[i], rr, P.rate);
        else if (rate && rr != rate) fail("bpeval: " + refs[i] + " has " + std::to_string(rr) + " Hz, the others " + std::to_string(rate) + " Hz");
        rate = P.rate ? P.rate : rr;
        if (a.size() > (size_t)INT32_MAX / 2) fail("bpeval: " + refs[i] + " is too long");
        if (P.rate) { both.push_back(a); both.push_back(b); both_rates.push_back(rr); both_rates.push_back(rr); continue; }
        r.insert(r.end(), a.begin(), a.end()); e.insert(e.end(), b.begin(), b.end());
        lens.push_back((int)a.size());
    }
    if (P.rate) {
        convert_rates(WHO, "pairs_list", P.device, P.rate, both, both_rates);
        for (size_t i = 0; i < both.size(); i += 2) {
            r.insert(r.end(), both[i].begin(), both[i].end()); e.insert(e.end(), both[i + 1].begin(), both[i + 1].end());
            lens.push_back((int)both[i].size());
        }
    }
    check_rate(rate);
    FILE *fo = nullptr;
    if (!P.scores_out.empty() && !(fo = fopen(P.scores_out.c_str(), "wt"))) fail("can not open scores file: " + P.scores_out);
    const int ns = n_columns(P.ext);
    std::vector<float> sc(lens.size() * ns);
    if (P.ext) check(bp_score_waves_ext(P.device, P.fea_dim, rate, (int)lens.size(), lens.data(), r.data(), e.data(), ns, sc.data()));
    else check(bp_score_waves(P.device, P.fea_dim, rate, (int)lens.size(), lens.data(), r.data(), e.data(), sc.data()));
    Acc a;
    for (size_t i = 0; i < lens.size(); ++i) {
        const float *s = &sc[i * ns];
        add(a, ns, s, s);
        if (!fo) continue;
        fprintf(fo, "%s %s", refs[i].c_str(), ests[i].c_str());
        put_scores(fo, ns, s);
        fprintf(fo, "\n");
    }
    if (fo) fclose(fo);
    printf("pairs: %d pairs", a.n);
    put_means(ns, a, false);
    printf(" (%d undefined)\n", a.nan / 2);
    return 1;
}

}  // namespace

int main(int argc, char **argv)
{
    const Params P = parse(argc, argv);
    const int D = P.fea_dim;
    check_fea_dim(WHO, D);
    if (!P.pairs_list.empty()) return pairs_mode(P);

    const int L = P.numlayers, ctx = P.fea_context, toff = P.targ_offset, hop = D - 1;
    if (L < 2) fail("bpeval: layersizes: need 2.." + std::to_string(BP_MAXLAYER - 1) + " layer sizes");
    if (P.norm_file.empty() || P.initwts_file.empty()) fail("bpeval: need norm_file and initwts_file");
    if (toff >= ctx) fail("bpeval: targ_offset must be below fea_context");
    if (P.layersizes[0] != ctx * D && P.layersizes[0] != (ctx + 1) * D) fail("bpeval: layersizes[0] must be fea_context*fea_dim (+ fea_dim with NAT)");
    if (P.layersizes[L - 1] != D && P.layersizes[L - 1] != 2 * D) fail("bpeval: layersizes[last] must be fea_dim or 2*fea_dim");
    if (P.out_col + D > P.layersizes[L - 1]) fail("bpeval: out_col + fea_dim exceeds layersizes[last]");
    if (P.snr.empty()) fail("bpeval: snr_list is empty");
    check_post_keys(WHO, P.post, P.wave_target);
    if (!P.gv_out.empty()) {
        if (P.post.on()) fail("bpeval: gv_out takes no post_gv or post_mask_col (the factors are those of the net's own columns)");
        if (P.wave_target != BP_WAVE_LPS) fail("bpeval: gv_out needs wave_target=lps");
        if (P.baseline || !P.scores_out.empty()) fail("bpeval: gv_out scores nothing: it takes no baseline or scores_out");
    }
    // every list and WAV is read and checked before the device is used
    int rate = 0;
    const Corpus clean = flatten(read_wav_list(WHO, "clean_list", P.clean_list, nullptr, &rate, P.rate, P.device));
    const Corpus noise = flatten(read_wav_list(WHO, "noise_list", P.noise_list, nullptr, &rate, P.rate, P.device));
    Reverb rv;                                                   // rir_list: the responses, at the rate of the others
    if (!P.rir_list.empty()) {
        const std::vector<std::string> paths = read_lines(WHO, "rir_list", P.rir_list);
        for (size_t k = 0; k < paths.size(); ++k) {
            int rr = 0;
            if (P.rate && (read_one(WHO, paths[k], &rr), rr != P.rate))
                fail("bpeval: rir_list: " + paths[k] + " has " + std::to_string(rr) + " Hz and rate=" + std::to_string(P.rate) +
                     " does not convert impulse responses (resampling one also rescales it)");
            const std::vector<float> w = read_one(WHO, paths[k], &rate);
            if (w.size() > (size_t)BP_MIX_RIR_MAX_TAPS) fail("bpeval: rir_list: " + paths[k] + " has more than " + std::to_string(BP_MIX_RIR_MAX_TAPS) + " taps");
            rv.pcm.insert(rv.pcm.end(), w.begin(), w.end());
            rv.len.push_back((int)w.size());
        }
    }
    check_rate(rate);
    check_rir_keys(WHO, P.rir, P.rir_list, "", " (cv_rir_rooms is bpmix's)");
    if (P.rir.rooms) {                                           // rir_rooms: drawn and checked here, made on the device by set_reverb
        std::string err = rir_draw(P.rir, P.seed, P.rir.rooms, rate, rv.rooms, rv.len);
        if (err.empty() && !P.rir.rooms_out.empty()) err = rir_write_rooms(P.rir.rooms_out, rv.rooms);
        if (!err.empty()) fail("bpeval: " + err);
    }
    rv.on = !rv.len.empty(); rv.target = P.reverb_target; rv.early_taps = early_taps(P.early_ms, rate); rv.rate = rate;
    check_noise(WHO, noise);
    const int n_clean = (int)clean.len.size();
    std::vector<bp_mixture> plan = make_plan(P.seed, n_clean, P.mix_per_clean, noise, P.snr);
    const auto calls = cut(WHO, plan, clean, hop, ctx, P.traincache);
    address_reverberant(plan, rv, n_clean);
    std::vector<float> mean, istd;
    read_norm(P.norm_file, D, mean, istd);
    Weights wts(L, P.layersizes);
    {
        const std::string err = load_weights(P.initwts_file, L, P.layersizes, wts);
        if (!err.empty()) fail(err);
    }
    FILE *fo = nullptr;
    if (!P.scores_out.empty() && !(fo = fopen(P.scores_out.c_str(), "wt"))) fail("can not open scores file: " + P.scores_out);

    bp_config cfg = net_config(L, P.layersizes, P.bunchsize, P.traincache, P.device);
    cfg.dropoutflag = P.dropoutflag; cfg.visible_omit = P.visible_omit; cfg.hid_omit = P.hid_omit;
    cfg.activation = P.activation; cfg.compute_dtype = P.compute_dtype;
    bp_handle *h = create_net(cfg, wts, P.output_act, P.output_linear_dims, P.output_loss);
    set_nat(WHO, h, P.nat, ctx, D, P.layersizes);
    set_post(h, P.post, D);
    const bp_mix_corpus mc = describe(D, ctx, toff, P.layersizes[L - 1] == D ? BP_MIX_LPS : BP_MIX_LPS_IRM, 5.0f, mean.data(), istd.data(), clean, noise);
    check(bp_set_mix_corpus(h, &mc));
    if (rv.on) set_reverb(h, P.rir, P.device, rv, P.seed, n_clean);
    if (!P.gv_out.empty()) {                                     // the GV factors of the net on this test set; nothing is scored
        std::vector<double> sums((size_t)4 * D, 0.0), part((size_t)4 * D);
        int64_t frames = 0;
        for (const auto &c : calls) {
            int64_t f = 0;
            check(bp_gv_mix(h, c.second - c.first, plan.data() + c.first, P.out_col, BP_GV_RAW, &part[0], &part[D], &part[2 * (size_t)D],
                            &part[3 * (size_t)D], &f));
            for (size_t k = 0; k < sums.size(); ++k) sums[k] += part[k];
            frames += f;
        }
        bp_destroy(h);
        std::vector<float> center(D), scale(D);
        check(bp_gv_factors(D, frames, &sums[0], &sums[D], &sums[2 * (size_t)D], &sums[3 * (size_t)D], P.gv_mode, center.data(), scale.data()));
        write_gv(P.gv_out, center, scale);
        if (P.gv_mode == BP_GV_INDEP)
            printf("bpeval: GV factor %.9g (indep) of %lld frames of %zu mixtures -> %s\n", scale[0], (long long)frames, plan.size(), P.gv_out.c_str());
        else
            printf("bpeval: GV factors %.9g .. %.9g (dep) of %lld frames of %zu mixtures -> %s\n", *std::min_element(scale.begin(), scale.end()),
                   *std::max_element(scale.begin(), scale.end()), (long long)frames, plan.size(), P.gv_out.c_str());
        return 1;
    }
    std::map<float, Acc> by_snr, by_snr_lm;
    Acc all, all_lm;
    std::vector<float> ns, es, ls;
    const int NS = n_columns(P.ext);
    for (const auto &c : calls) {
        const int n = c.second - c.first;
        const bp_mixture *pm = plan.data() + c.first;
        ns.resize((size_t)n * NS); es.resize((size_t)n * NS);
        if (P.ext) check(bp_eval_mix_ext(h, n, pm, rate, P.wave_target, P.out_col, NS, ns.data(), es.data(), nullptr));
        else check(bp_eval_mix(h, n, pm, rate, P.wave_target, P.out_col, ns.data(), es.data(), nullptr));
        if (P.baseline) {                                    // (its noisy scores are those of bp_eval_mix: ns is written twice)
            ls.resize((size_t)n * NS);
            if (P.lm_noise != BP_NOISE_VAD) {
                bp_noise_params nz;
                bp_noise_defaults(&nz);
                nz.mode = P.lm_noise;
                check(bp_eval_mix_logmmse_nt(h, nullptr, &nz, n, pm, rate, NS, ns.data(), ls.data(), nullptr));
            }
            else if (P.ext) check(bp_eval_mix_logmmse_ext(h, nullptr, n, pm, rate, NS, ns.data(), ls.data(), nullptr));
            else check(bp_eval_mix_logmmse(h, nullptr, n, pm, rate, ns.data(), ls.data(), nullptr));
        }
        for (int i = 0; i < n; ++i) {
            const bp_mixture &m = plan[c.first + i];
            const float *a = &ns[(size_t)i * NS], *b = &es[(size_t)i * NS];
            add(by_snr[m.snr_db], NS, a, b); add(all, NS, a, b);
            if (fo) {
                fprintf(fo, "%d %d %lld %.9g", m.clean, m.noise, (long long)m.offset, m.snr_db);
                put_scores(fo, NS, a, b);
            }
            if (P.baseline) {
                const float *l = &ls[(size_t)i * NS];
                add(by_snr_lm[m.snr_db], NS, a, l); add(all_lm, NS, a, l);
                if (fo) put_scores(fo, NS, l);
            }
            if (fo) fprintf(fo, "\n");
        }
    }
    bp_destroy(h);
    if (fo) fclose(fo);
    const auto line = [NS](const char *head, const char *who, const Acc &a) {       // who: "" or "logmmse: "
        printf("%s: %d mixtures", head, a.n);
        put_means(NS, a, true, who);
        printf(" (%d undefined)\n", a.nan);
    };
    for (const auto &kv : by_snr) {
        char head[64];
        snprintf(head, sizeof(head), "SNR %g dB", kv.first);
        line(head, "", kv.second);
        if (P.baseline) line(head, "logmmse: ", by_snr_lm[kv.first]);
    }
    line("all", "", all);
    if (P.baseline) line("all", "logmmse: ", all_lm);
    return 1;
}
