// bpeval.cpp -- objective scores of enhanced speech on the MI355X: segmental SNR, log-spectral distortion and
// STOI, through bp_eval_mix (a test set mixed on the GPU and enhanced with a trained net) or bp_score_waves (pairs of WAVs).
//
//   bpeval clean_list=test_clean.list noise_list=test_noise.list norm_file=x.norm initwts_file=mlp.N.wts fea_dim=129 fea_context=11
//          targ_offset=5 layersizes=1548,2048,2048,2048,129 [snr_list=-5,0,5,10,15,20] [mix_per_clean=1] [init_randem_seed=0]
//          [wave_target=lps|mask] [out_col=0] [traincache=102400] [bunchsize=1024] [dropoutflag=1 visible_omit=0.1 hid_omit=0.2]
//          [activation=relu|sigmoid] [compute=fp32|bf16] [output_act=... output_linear_dims=... output_loss=...] [device=0]
//          [scores_out=scores.txt] [baseline=logmmse] [rir_list=rir.list] [reverb_target=reverberant|early] [early_ms=50]
//   bpeval pairs_list=<"ref.wav est.wav" per line> fea_dim=129 [device=0] [scores_out=scores.txt]
//
// Test-set mode: the plan is bp_mix_plan(init_randem_seed, clean sentences, mix_per_clean, noise lengths, snr_list), cut into calls
// of at most traincache rows (frames + n_mix (context-1)) in plan order, as bpmix cuts it; every WAV must have the same rate.
// stdout: one line per SNR (ascending) and one "all:" line, noisy -> enhanced; means skip NaN, and the count of NaN scores of the
// line is printed.  scores_out: one line per mixture in plan order, `clean noise offset snr ssnr_noisy ssnr_enh lsd_noisy lsd_enh
// stoi_noisy stoi_enh` (%.9g: the floats round-trip); pairs mode: `ref est ssnr lsd stoi` per pair.  Every key, list and WAV is
// checked before the device is used.  baseline=logmmse (test-set mode only) scores the classic log-MMSE enhancer on the same
// mixtures beside the net (bp_eval_mix_logmmse): after every stdout line a second one with `logmmse:` in place of
// the net's figures (noisy -> logmmse), and three more columns `ssnr_lm lsd_lm stoi_lm` at the end of every scores_out line.
// rir_list: one room impulse response per WAV, at the rate of the others; clean sentence c is paired with response
// bp_mix_reverb_pairs(init_randem_seed, ...)[c], the plan addresses the derived entry n_clean + c in place of c (so scores_out
// lists it), the mixtures are reverberant and the scores are taken against reverb_target: the reverberant sentence or its direct
// sound + early_ms of reflections.  rir_rooms=N with rir_room_lo / rir_room_hi / rir_t60 / rir_margin / rir_dist / rir_ms / rir_window /
// rir_rooms_out (bpmix's keys, its defaults) takes the place of rir_list: N simulated responses, their rooms drawn
// by bp_rir_rooms(init_randem_seed, N, ...) and made by bp_rir_image at the rate of the others.
// Errors: message + exit(0); success: return 1 (reference convention).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../../include/bp_c_api.h"
#include "rir_keys.h"
#include "wav_io.h"
#include "wts_io.h"

namespace {

[[noreturn]] void die(const std::string &msg)
{
    printf("%s\n", msg.c_str());
    exit(0);
}

void check(int rc)
{
    if (rc != 0) die(bp_last_error());
}

struct Params {
    std::string clean_list, noise_list, pairs_list, norm_file, initwts_file, scores_out, rir_list;
    int reverb_target = BP_REVERB_TARGET_REVERBERANT;
    float early_ms = 50.0f;
    int fea_dim = 0, fea_context = 1, targ_offset = 0, dropoutflag = 0, traincache = 102400, bunchsize = 1024, numlayers = 0;
    int layersizes[BP_MAXLAYER] = {0}, mix_per_clean = 1, activation = 0, compute_dtype = 0, device = 0;
    int output_act = 0, output_linear_dims = 0, output_loss = 0, wave_target = BP_WAVE_LPS, out_col = 0;
    float visible_omit = 0, hid_omit = 0;
    unsigned long long seed = 0;
    std::vector<float> snr = {-5, 0, 5, 10, 15, 20};
    bool net_keys = false;                                   // a key of test-set mode was given
    bool baseline = false;                                   // baseline=logmmse
    bp::RirKeys rir;                                         // rir_rooms=N ...: simulated responses in place of rir_list
};

bool parse_int(const std::string &v, long lo, long hi, int *out)
{
    char *end = nullptr;
    const long n = strtol(v.c_str(), &end, 10);
    if (v.empty() || *end || n < lo || n > hi) return false;
    *out = (int)n;
    return true;
}
bool parse_float(const std::string &v, float *out)
{
    char *end = nullptr;
    const double d = strtod(v.c_str(), &end);
    if (v.empty() || *end || !std::isfinite(d)) return false;
    *out = (float)d;
    return true;
}

Params parse(int argc, char **argv)
{
    Params P;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) die(std::string("Arg: ") + argv[i] + "  Format Error");
        const std::string k(argv[i], eq - argv[i]), v(eq + 1);
        bool ok = true, net = true;
        if (k == "pairs_list") { P.pairs_list = v; net = false; }
        else if (k == "scores_out") { P.scores_out = v; net = false; }
        else if (k == "fea_dim") { ok = parse_int(v, 1, 1 << 20, &P.fea_dim); net = false; }
        else if (k == "device") { ok = parse_int(v, 0, 1023, &P.device); net = false; }
        else if (k == "clean_list") P.clean_list = v; else if (k == "noise_list") P.noise_list = v;
        else if (k == "norm_file") P.norm_file = v; else if (k == "initwts_file") P.initwts_file = v;
        else if (k == "rir_list") P.rir_list = v;
        else if (k == "reverb_target") {
            if (v == "reverberant") P.reverb_target = BP_REVERB_TARGET_REVERBERANT; else if (v == "early") P.reverb_target = BP_REVERB_TARGET_EARLY;
            else die("reverb_target: " + v + " is not reverberant or early");
        }
        else if (k == "early_ms") ok = parse_float(v, &P.early_ms) && P.early_ms >= 0.0f && P.early_ms <= 1e6f;
        else if (k == "fea_context") ok = parse_int(v, 1, 1000, &P.fea_context);
        else if (k == "targ_offset") ok = parse_int(v, 0, 999, &P.targ_offset);
        else if (k == "dropoutflag") ok = parse_int(v, 0, 1, &P.dropoutflag);
        else if (k == "traincache") ok = parse_int(v, 1, BP_MAXCACHEFRAME, &P.traincache);
        else if (k == "bunchsize") ok = parse_int(v, 1, 1 << 20, &P.bunchsize);
        else if (k == "mix_per_clean") ok = parse_int(v, 1, 1 << 20, &P.mix_per_clean);
        else if (k == "out_col") ok = parse_int(v, 0, 1 << 20, &P.out_col);
        else if (k == "output_linear_dims") ok = parse_int(v, 0, 1000000, &P.output_linear_dims);
        else if (k == "visible_omit") ok = parse_float(v, &P.visible_omit); else if (k == "hid_omit") ok = parse_float(v, &P.hid_omit);
        else if (k == "init_randem_seed") {
            char *end = nullptr;
            P.seed = strtoull(v.c_str(), &end, 10);
            ok = !v.empty() && !*end && v[0] != '-';
        } else if (k == "layersizes") {
            P.numlayers = 0;
            size_t pos = 0;
            while (ok) {
                const size_t c = v.find(',', pos);
                if (P.numlayers == BP_MAXLAYER - 1) { ok = false; break; }
                ok = parse_int(v.substr(pos, c == std::string::npos ? c : c - pos), 1, 1 << 20, &P.layersizes[P.numlayers++]);
                if (c == std::string::npos) break;
                pos = c + 1;
            }
        } else if (k == "snr_list") {
            P.snr.clear();
            size_t pos = 0;
            while (ok) {
                const size_t c = v.find(',', pos);
                float s = 0;
                ok = parse_float(v.substr(pos, c == std::string::npos ? c : c - pos), &s);
                P.snr.push_back(s);
                if (c == std::string::npos) break;
                pos = c + 1;
            }
        }
        else if (k == "baseline") { if (v == "logmmse") P.baseline = true; else ok = false; }
        else if (k == "wave_target") { if (v == "lps") P.wave_target = BP_WAVE_LPS; else if (v == "mask") P.wave_target = BP_WAVE_MASK; else ok = false; }
        else if (k == "activation") { if (v == "relu") P.activation = 0; else if (v == "sigmoid") P.activation = 1; else ok = false; }
        else if (k == "compute") { if (v == "fp32") P.compute_dtype = 0; else if (v == "bf16") P.compute_dtype = 1; else ok = false; }
        else if (k == "output_act") { if (v == "linear") P.output_act = 0; else if (v == "sigmoid") P.output_act = 1; else ok = false; }
        else if (k == "output_loss") { if (v == "xent") P.output_loss = 0; else if (v == "mse") P.output_loss = 1; else ok = false; }
        else if (const int r = bp::rir_key(P.rir, k, v)) ok = r > 0;
        else die("bpeval: unknown key " + k);
        if (!ok) die("bpeval: bad value for " + k + ": " + v);
        P.net_keys = P.net_keys || net;
    }
    return P;
}

std::string trim(std::string s)
{
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ' || s.back() == '\t')) s.pop_back();
    size_t i = 0;
    while (i < s.size() && (s[i] == ' ' || s[i] == '\t')) ++i;
    return s.substr(i);
}

std::vector<std::string> read_lines(const std::string &what, const std::string &list)
{
    if (list.empty()) die("bpeval: " + what + " is not given");
    FILE *fl = fopen(list.c_str(), "rt");
    if (!fl) die("can not open " + what + ": " + list);
    std::vector<std::string> out;
    char line[8192];
    while (fgets(line, sizeof(line), fl)) {
        const std::string t = trim(line);
        if (!t.empty()) out.push_back(t);
    }
    fclose(fl);
    if (out.empty()) die("bpeval: " + list + " lists no wav file");
    return out;
}

// one WAV, non-empty, at the rate of the others (*rate = 0: the first one sets it)
std::vector<float> read_one(const std::string &path, int *rate)
{
    std::vector<float> w;
    int sr = 0;
    const std::string err = bp::read_wav(path, w, sr);
    if (!err.empty()) die(err);
    if (w.empty()) die(path + ": no samples");
    if (*rate && sr != *rate) die("bpeval: " + path + " has " + std::to_string(sr) + " Hz, the others " + std::to_string(*rate) + " Hz");
    *rate = sr;
    return w;
}

struct Corpus {
    std::vector<float> pcm;
    std::vector<int64_t> len;
};
Corpus read_corpus(const std::string &what, const std::string &list, int *rate)
{
    Corpus c;
    for (const std::string &p : read_lines(what, list)) {
        const std::vector<float> w = read_one(p, rate);
        c.pcm.insert(c.pcm.end(), w.begin(), w.end());
        c.len.push_back((int64_t)w.size());
    }
    return c;
}

void check_rate(int fs)
{
    int a = 10000, b = fs;
    while (b) { const int t = a % b; a = b; b = t; }
    if (fs <= 0 || 10000 / a > 32 || fs / a > 32)
        die("bpeval: " + std::to_string(fs) + " Hz is not a scoring rate (8, 10, 12, 16, 20, 24, 32, 48 kHz)");
}

// mean over the finite values; NaN count
struct Acc { double sum[BP_SCORE_N * 2] = {0}; int cnt[BP_SCORE_N * 2] = {0}, n = 0, nan = 0; };
void add(Acc &a, const float *noisy, const float *enh)
{
    ++a.n;
    for (int k = 0; k < 2 * BP_SCORE_N; ++k) {
        const float v = k < BP_SCORE_N ? noisy[k] : enh[k - BP_SCORE_N];
        if (std::isnan(v)) { ++a.nan; continue; }
        a.sum[k] += v; ++a.cnt[k];
    }
}
double avg(const Acc &a, int k) { return a.cnt[k] ? a.sum[k] / a.cnt[k] : NAN; }

void read_norm(const std::string &path, int D, std::vector<float> &mean, std::vector<float> &istd)
{
    FILE *fn = fopen(path.c_str(), "rt");
    if (!fn) die("can not open normalization file: " + path);
    char buff[1024];
    mean.assign(D, 0.f); istd.assign(D, 0.f);
    bool ok = fgets(buff, sizeof(buff), fn) != nullptr;
    for (int j = 0; ok && j < D; ++j) { ok = fgets(buff, sizeof(buff), fn) != nullptr; mean[j] = (float)atof(buff); }
    ok = ok && fgets(buff, sizeof(buff), fn) != nullptr;
    for (int j = 0; ok && j < D; ++j) { ok = fgets(buff, sizeof(buff), fn) != nullptr; istd[j] = (float)atof(buff); }
    fclose(fn);
    if (!ok) die("normalization file too short");
}

int pairs_mode(const Params &P)
{
    if (P.net_keys) die("bpeval: pairs_list takes only fea_dim, device and scores_out");   // (baseline= counts as a key of test-set mode)
    std::vector<std::string> refs, ests;
    for (const std::string &t : read_lines("pairs_list", P.pairs_list)) {
        const size_t sp = t.find_first_of(" \t");
        if (sp == std::string::npos) die("pairs list " + P.pairs_list + ": line \"" + t + "\" needs a reference and an estimate");
        refs.push_back(t.substr(0, sp)); ests.push_back(trim(t.substr(sp)));
    }
    std::vector<float> r, e;
    std::vector<int> lens;
    int rate = 0;
    for (size_t i = 0; i < refs.size(); ++i) {
        int rr = 0, re = 0;
        const std::vector<float> a = read_one(refs[i], &rr), b = read_one(ests[i], &re);
        if (rr != re) die("bpeval: " + refs[i] + " and " + ests[i] + " differ in sample rate");
        if (a.size() != b.size()) die("bpeval: " + refs[i] + " and " + ests[i] + " differ in length");
        if (rate && rr != rate) die("bpeval: " + refs[i] + " has " + std::to_string(rr) + " Hz, the others " + std::to_string(rate) + " Hz");
        rate = rr;
        if (a.size() > (size_t)INT32_MAX / 2) die("bpeval: " + refs[i] + " is too long");
        r.insert(r.end(), a.begin(), a.end()); e.insert(e.end(), b.begin(), b.end());
        lens.push_back((int)a.size());
    }
    check_rate(rate);
    FILE *fo = nullptr;
    if (!P.scores_out.empty() && !(fo = fopen(P.scores_out.c_str(), "wt"))) die("can not open scores file: " + P.scores_out);
    std::vector<float> sc(lens.size() * BP_SCORE_N);
    check(bp_score_waves(P.device, P.fea_dim, rate, (int)lens.size(), lens.data(), r.data(), e.data(), sc.data()));
    Acc a;
    for (size_t i = 0; i < lens.size(); ++i) {
        const float *s = &sc[i * BP_SCORE_N];
        add(a, s, s);
        if (fo) fprintf(fo, "%s %s %.9g %.9g %.9g\n", refs[i].c_str(), ests[i].c_str(), s[0], s[1], s[2]);
    }
    if (fo) fclose(fo);
    printf("pairs: %d pairs, SSNR %.3f dB, LSD %.3f dB, STOI %.4f (%d undefined)\n", a.n, avg(a, BP_SCORE_SSNR), avg(a, BP_SCORE_LSD),
           avg(a, BP_SCORE_STOI), a.nan / 2);
    return 1;
}

}  // namespace

int main(int argc, char **argv)
{
    const Params P = parse(argc, argv);
    const int D = P.fea_dim, n_fft = 2 * (D - 1);
    if (D < 33 || D > 1025 || (n_fft & (n_fft - 1))) die("bpeval: fea_dim must make 2*(fea_dim-1) a power of two from 64 to 2048");
    if (!P.pairs_list.empty()) return pairs_mode(P);

    const int L = P.numlayers, ctx = P.fea_context, toff = P.targ_offset, hop = D - 1;
    if (L < 2) die("bpeval: layersizes: need 2.." + std::to_string(BP_MAXLAYER - 1) + " layer sizes");
    if (P.norm_file.empty() || P.initwts_file.empty()) die("bpeval: need norm_file and initwts_file");
    if (toff >= ctx) die("bpeval: targ_offset must be below fea_context");
    if (P.layersizes[0] != ctx * D && P.layersizes[0] != (ctx + 1) * D) die("bpeval: layersizes[0] must be fea_context*fea_dim (+ fea_dim with NAT)");
    if (P.layersizes[L - 1] != D && P.layersizes[L - 1] != 2 * D) die("bpeval: layersizes[last] must be fea_dim or 2*fea_dim");
    if (P.out_col + D > P.layersizes[L - 1]) die("bpeval: out_col + fea_dim exceeds layersizes[last]");
    if (P.snr.empty()) die("bpeval: snr_list is empty");
    // every list and WAV is read and checked before the device is used
    int rate = 0;
    const Corpus clean = read_corpus("clean_list", P.clean_list, &rate);
    const Corpus noise = read_corpus("noise_list", P.noise_list, &rate);
    std::vector<float> rir_pcm;                                  // rir_list: the responses, at the rate of the others
    std::vector<int> rir_len;
    if (!P.rir_list.empty()) {
        const std::vector<std::string> paths = read_lines("rir_list", P.rir_list);
        for (size_t k = 0; k < paths.size(); ++k) {
            const std::vector<float> w = read_one(paths[k], &rate);
            if (w.size() > (size_t)BP_MIX_RIR_MAX_TAPS) die("bpeval: rir_list: " + paths[k] + " has more than " + std::to_string(BP_MIX_RIR_MAX_TAPS) + " taps");
            rir_pcm.insert(rir_pcm.end(), w.begin(), w.end());
            rir_len.push_back((int)w.size());
        }
    }
    check_rate(rate);
    std::vector<bp_rir_room> rooms;                              // rir_rooms: drawn and checked here, made on the device below
    if (P.rir.rooms && !P.rir_list.empty()) die("bpeval: rir_rooms and rir_list exclude each other");
    if ((P.rir.any || P.rir.cv_rooms) && !P.rir.rooms) die("bpeval: the rir_* keys need rir_rooms (cv_rir_rooms is bpmix's)");
    if (P.rir.rooms) {
        std::string err = bp::rir_draw(P.rir, P.seed, P.rir.rooms, rate, rooms, rir_len);
        if (err.empty() && !P.rir.rooms_out.empty()) err = bp::rir_write_rooms(P.rir.rooms_out, rooms);
        if (!err.empty()) die("bpeval: " + err);
    }
    for (int64_t n : noise.len)
        if (n >= ((int64_t)1 << 32)) die("bpeval: a noise recording has 2^32 samples or more");
    std::vector<bp_mixture> plan((size_t)clean.len.size() * P.mix_per_clean);
    check(bp_mix_plan(P.seed, (int)clean.len.size(), P.mix_per_clean, (int)noise.len.size(), noise.len.data(), (int)P.snr.size(),
                      P.snr.data(), plan.data()));
    // calls of at most traincache rows, consecutive mixtures of the plan (bpmix's cut)
    std::vector<std::pair<int, int>> calls;
    {
        int first = 0;
        long rows = 0;
        for (int m = 0; m < (int)plan.size(); ++m) {
            const long T = (long)((clean.len[plan[m].clean] - 1) / hop + 2);
            if (T + ctx - 1 > P.traincache) die("bpeval: clean sentence " + std::to_string(plan[m].clean) + " does not fit one chunk of traincache frames");
            if (rows + T + ctx - 1 > P.traincache) { calls.push_back({first, m}); first = m; rows = 0; }
            rows += T + ctx - 1;
        }
        calls.push_back({first, (int)plan.size()});
    }
    const int n_clean = (int)clean.len.size();
    if (!rir_len.empty()) for (bp_mixture &m : plan) m.clean += n_clean;            // (the derived entry of sentence c: n_clean + c)
    std::vector<float> mean, istd;
    read_norm(P.norm_file, D, mean, istd);
    std::vector<std::vector<float>> Wv(L), Bv(L);
    float *weights[BP_MAXLAYER] = {0}, *bias[BP_MAXLAYER] = {0};
    for (int i = 1; i < L; ++i) {
        Wv[i].assign((size_t)P.layersizes[i] * P.layersizes[i - 1], 0.f); Bv[i].assign(P.layersizes[i], 0.f);
        weights[i] = Wv[i].data(); bias[i] = Bv[i].data();
    }
    {
        FILE *fi = fopen(P.initwts_file.c_str(), "rb");
        if (!fi) die("can not open initial weights file: " + P.initwts_file);
        const std::string err = bp::read_weights(fi, L, P.layersizes, weights, bias);
        fclose(fi);
        if (!err.empty()) die(err);
    }
    FILE *fo = nullptr;
    if (!P.scores_out.empty() && !(fo = fopen(P.scores_out.c_str(), "wt"))) die("can not open scores file: " + P.scores_out);

    bp_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.gpu_used = 1; cfg.numlayers = L;
    for (int i = 0; i < L; ++i) cfg.layersizes[i] = P.layersizes[i];
    cfg.bunchsize = P.bunchsize; cfg.dropoutflag = P.dropoutflag; cfg.visible_omit = P.visible_omit; cfg.hid_omit = P.hid_omit;
    cfg.activation = P.activation; cfg.compute_dtype = P.compute_dtype; cfg.max_chunk_frames = P.traincache; cfg.device = P.device;
    bp_handle *h = nullptr;
    check(bp_create(&cfg, weights, bias, &h));
    check(bp_set_output(h, P.output_act, P.output_linear_dims, P.output_loss));
    bp_mix_corpus mc;
    memset(&mc, 0, sizeof(mc));
    mc.fea_dim = D; mc.context = ctx; mc.targ_offset = toff; mc.target = P.layersizes[L - 1] == D ? BP_MIX_LPS : BP_MIX_LPS_IRM;
    mc.lc_db = 5.0f; mc.mean = mean.data(); mc.inv_std = istd.data();
    mc.n_clean = (int)clean.len.size(); mc.clean_len = clean.len.data(); mc.clean_pcm = clean.pcm.data();
    mc.n_noise = (int)noise.len.size(); mc.noise_len = noise.len.data(); mc.noise_pcm = noise.pcm.data();
    check(bp_set_mix_corpus(h, &mc));
    if (!rooms.empty()) {
        const std::string err = bp::rir_generate(P.rir, P.device, rate, rooms, rir_len, rir_pcm);
        if (!err.empty()) die(err);
    }
    if (!rir_len.empty()) {
        std::vector<int> pc(n_clean), pr(n_clean);
        for (int c = 0; c < n_clean; ++c) pc[c] = c;
        check(bp_mix_reverb_pairs(P.seed, n_clean, (int)rir_len.size(), pr.data()));
        bp_mix_reverb mr;
        memset(&mr, 0, sizeof(mr));
        mr.n_rir = (int)rir_len.size(); mr.rir_len = rir_len.data(); mr.rir_pcm = rir_pcm.data();
        mr.n_pair = n_clean; mr.pair_clean = pc.data(); mr.pair_rir = pr.data();
        mr.target = P.reverb_target; mr.early_taps = (int)((double)P.early_ms * rate / 1000.0 + 0.5);
        check(bp_set_mix_reverb(h, &mr));
    }
    std::map<float, Acc> by_snr, by_snr_lm;
    Acc all, all_lm;
    std::vector<float> ns, es, ls;
    for (const auto &c : calls) {
        const int n = c.second - c.first;
        ns.resize((size_t)n * BP_SCORE_N); es.resize((size_t)n * BP_SCORE_N);
        check(bp_eval_mix(h, n, plan.data() + c.first, rate, P.wave_target, P.out_col, ns.data(), es.data(), nullptr));
        if (P.baseline) {                                    // (its noisy scores are those of bp_eval_mix: ns is written twice)
            ls.resize((size_t)n * BP_SCORE_N);
            check(bp_eval_mix_logmmse(h, nullptr, n, plan.data() + c.first, rate, ns.data(), ls.data(), nullptr));
        }
        for (int i = 0; i < n; ++i) {
            const bp_mixture &m = plan[c.first + i];
            const float *a = &ns[(size_t)i * BP_SCORE_N], *b = &es[(size_t)i * BP_SCORE_N];
            add(by_snr[m.snr_db], a, b); add(all, a, b);
            if (fo)
                fprintf(fo, "%d %d %lld %.9g %.9g %.9g %.9g %.9g %.9g %.9g", m.clean, m.noise, (long long)m.offset, m.snr_db,
                        a[BP_SCORE_SSNR], b[BP_SCORE_SSNR], a[BP_SCORE_LSD], b[BP_SCORE_LSD], a[BP_SCORE_STOI], b[BP_SCORE_STOI]);
            if (P.baseline) {
                const float *l = &ls[(size_t)i * BP_SCORE_N];
                add(by_snr_lm[m.snr_db], a, l); add(all_lm, a, l);
                if (fo) fprintf(fo, " %.9g %.9g %.9g", l[BP_SCORE_SSNR], l[BP_SCORE_LSD], l[BP_SCORE_STOI]);
            }
            if (fo) fprintf(fo, "\n");
        }
    }
    bp_destroy(h);
    if (fo) fclose(fo);
    const auto line = [](const char *head, const Acc &a) {
        printf("%s: %d mixtures, SSNR %.3f -> %.3f dB, LSD %.3f -> %.3f dB, STOI %.4f -> %.4f (%d undefined)\n", head, a.n,
               avg(a, BP_SCORE_SSNR), avg(a, BP_SCORE_N + BP_SCORE_SSNR), avg(a, BP_SCORE_LSD), avg(a, BP_SCORE_N + BP_SCORE_LSD),
               avg(a, BP_SCORE_STOI), avg(a, BP_SCORE_N + BP_SCORE_STOI), a.nan);
    };
    const auto line_lm = [](const char *head, const Acc &a) {
        printf("%s: %d mixtures, logmmse: SSNR %.3f -> %.3f dB, LSD %.3f -> %.3f dB, STOI %.4f -> %.4f (%d undefined)\n", head, a.n,
               avg(a, BP_SCORE_SSNR), avg(a, BP_SCORE_N + BP_SCORE_SSNR), avg(a, BP_SCORE_LSD), avg(a, BP_SCORE_N + BP_SCORE_LSD),
               avg(a, BP_SCORE_STOI), avg(a, BP_SCORE_N + BP_SCORE_STOI), a.nan);
    };
    for (const auto &kv : by_snr) {
        char head[64];
        snprintf(head, sizeof(head), "SNR %g dB", kv.first);
        line(head, kv.second);
        if (P.baseline) line_lm(head, by_snr_lm[kv.first]);
    }
    line("all", all);
    if (P.baseline) line_lm("all", all_lm);
    return 1;
}
