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
//         [rir_window=taps] [rir_rooms_out=rooms.txt] [cv_rir_rooms=N]
//   bpmix clean_list=... noise_list=... fea_dim=129 norm_out=mix.norm [snr_list=...] [mix_per_clean=...] [init_randem_seed=...]
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
// Every key, list, WAV and drawn room is checked before the device is used.  Errors: message +
// exit(0); success: return 1 (reference convention).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

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
    std::string clean_list, noise_list, cv_clean_list, cv_noise_list, norm_file, norm_out, mix_plan_out;
    std::string initwts_file, outwts_file, log_file, rir_list, cv_rir_list;
    int reverb_target = BP_REVERB_TARGET_REVERBERANT;
    float early_ms = 50.0f;
    int fea_dim = 0, fea_context = 1, targ_offset = 0, dropoutflag = 0, traincache = 0, bunchsize = 0, numlayers = 0;
    int layersizes[BP_MAXLAYER] = {0}, mix_per_clean = 1, target = BP_MIX_LPS, activation = 0, momentum_rule = 0, compute_dtype = 0;
    int output_act = 0, output_linear_dims = 0, output_loss = 0, device = 0;
    float momentum = 0, weightcost = 0, lrate = 0, visible_omit = 0, hid_omit = 0, lc_db = 5.0f;
    float wmin = -0.1f, wmax = 0.1f, bmin = -0.1f, bmax = 0.1f;
    unsigned long long seed = 0, cv_seed = 20261016ull, dropout_seed = 0;
    std::vector<float> snr = {-5, 0, 5, 10, 15, 20};
    bp::RirKeys rir;
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
bool parse_u64(const std::string &v, unsigned long long *out)
{
    char *end = nullptr;
    const unsigned long long n = strtoull(v.c_str(), &end, 10);
    if (v.empty() || *end || v[0] == '-') return false;
    *out = n;
    return true;
}

Params parse(int argc, char **argv)
{
    Params P;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) die(std::string("Arg: ") + argv[i] + "  Format Error");
        const std::string k(argv[i], eq - argv[i]), v(eq + 1);
        bool ok = true;
        if (k == "clean_list") P.clean_list = v; else if (k == "noise_list") P.noise_list = v;
        else if (k == "cv_clean_list") P.cv_clean_list = v; else if (k == "cv_noise_list") P.cv_noise_list = v;
        else if (k == "norm_file") P.norm_file = v; else if (k == "norm_out") P.norm_out = v; else if (k == "mix_plan_out") P.mix_plan_out = v;
        else if (k == "initwts_file") P.initwts_file = v; else if (k == "outwts_file") P.outwts_file = v; else if (k == "log_file") P.log_file = v;
        else if (k == "rir_list") P.rir_list = v; else if (k == "cv_rir_list") P.cv_rir_list = v;
        else if (k == "reverb_target") {
            if (v == "reverberant") P.reverb_target = BP_REVERB_TARGET_REVERBERANT; else if (v == "early") P.reverb_target = BP_REVERB_TARGET_EARLY;
            else die("reverb_target: " + v + " is not reverberant or early");
        }
        else if (k == "early_ms") ok = parse_float(v, &P.early_ms) && P.early_ms >= 0.0f && P.early_ms <= 1e6f;
        else if (k == "fea_dim") ok = parse_int(v, 1, 1 << 20, &P.fea_dim);
        else if (k == "fea_context") ok = parse_int(v, 1, 1000, &P.fea_context);
        else if (k == "targ_offset") ok = parse_int(v, 0, 999, &P.targ_offset);
        else if (k == "dropoutflag") ok = parse_int(v, 0, 1, &P.dropoutflag);
        else if (k == "traincache") ok = parse_int(v, 1, BP_MAXCACHEFRAME, &P.traincache);
        else if (k == "bunchsize") ok = parse_int(v, 1, 1 << 20, &P.bunchsize);
        else if (k == "numlayers") ok = parse_int(v, 2, BP_MAXLAYER - 1, &P.numlayers);
        else if (k == "gpu_used") { int g = 0; ok = parse_int(v, 1, 1, &g); }           // (one GPU: mixing is single-device)
        else if (k == "device") ok = parse_int(v, 0, 1023, &P.device);
        else if (k == "mix_per_clean") ok = parse_int(v, 1, 1 << 20, &P.mix_per_clean);
        else if (k == "init_randem_seed") ok = parse_u64(v, &P.seed);
        else if (k == "cv_seed") ok = parse_u64(v, &P.cv_seed);
        else if (k == "seed") ok = parse_u64(v, &P.dropout_seed);
        else if (k == "lrate") ok = parse_float(v, &P.lrate); else if (k == "momentum") ok = parse_float(v, &P.momentum);
        else if (k == "weightcost") ok = parse_float(v, &P.weightcost); else if (k == "visible_omit") ok = parse_float(v, &P.visible_omit);
        else if (k == "hid_omit") ok = parse_float(v, &P.hid_omit); else if (k == "lc_db") ok = parse_float(v, &P.lc_db);
        else if (k == "init_randem_weight_min") ok = parse_float(v, &P.wmin); else if (k == "init_randem_weight_max") ok = parse_float(v, &P.wmax);
        else if (k == "init_randem_bias_min") ok = parse_float(v, &P.bmin); else if (k == "init_randem_bias_max") ok = parse_float(v, &P.bmax);
        else if (k == "layersizes") {
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
        } else if (k == "target") {
            if (v == "lps") P.target = BP_MIX_LPS; else if (v == "irm") P.target = BP_MIX_IRM; else if (v == "ibm") P.target = BP_MIX_IBM;
            else if (v == "lps+irm") P.target = BP_MIX_LPS_IRM; else if (v == "lps+ibm") P.target = BP_MIX_LPS_IBM;
            else die("target: " + v + " is not lps, irm, ibm, lps+irm or lps+ibm");
        }
        else if (k == "activation") { if (v == "relu") P.activation = 0; else if (v == "sigmoid") P.activation = 1; else ok = false; }
        else if (k == "momentum_rule") { if (v == "live") P.momentum_rule = 0; else if (v == "classic") P.momentum_rule = 1; else ok = false; }
        else if (k == "compute") { if (v == "fp32") P.compute_dtype = 0; else if (v == "bf16") P.compute_dtype = 1; else ok = false; }
        else if (k == "output_act") { if (v == "linear") P.output_act = 0; else if (v == "sigmoid") P.output_act = 1; else ok = false; }
        else if (k == "output_linear_dims") ok = parse_int(v, 0, 1000000, &P.output_linear_dims);
        else if (k == "output_loss") { if (v == "xent") P.output_loss = 0; else if (v == "mse") P.output_loss = 1; else ok = false; }
        else if (const int r = bp::rir_key(P.rir, k, v)) ok = r > 0;
        else die("bpmix: unknown key " + k);
        if (!ok) die("bpmix: bad value for " + k + ": " + v);
    }
    return P;
}

std::vector<std::vector<float>> read_list(const std::string &what, const std::string &list, std::vector<int> *rates = nullptr)
{
    if (list.empty()) die("bpmix: " + what + " is not given");
    FILE *fl = fopen(list.c_str(), "rt");
    if (!fl) die("can not open " + what + ": " + list);
    std::vector<std::vector<float>> waves;
    char line[4096];
    while (fgets(line, sizeof(line), fl)) {
        std::string p(line);
        while (!p.empty() && (p.back() == '\n' || p.back() == '\r' || p.back() == ' ' || p.back() == '\t')) p.pop_back();
        if (p.empty()) continue;
        waves.emplace_back();
        int sr = 0;
        const std::string err = bp::read_wav(p, waves.back(), sr);
        if (!err.empty()) { fclose(fl); die(err); }
        if (waves.back().empty()) { fclose(fl); die(p + ": no samples"); }
        if (rates) rates->push_back(sr);
    }
    fclose(fl);
    if (waves.empty()) die("bpmix: " + list + " lists no wav file");
    return waves;
}

struct Corpus {
    std::vector<float> pcm;
    std::vector<int64_t> len;
};
Corpus flatten(const std::vector<std::vector<float>> &w)
{
    Corpus c;
    for (const auto &x : w) { c.pcm.insert(c.pcm.end(), x.begin(), x.end()); c.len.push_back((int64_t)x.size()); }
    return c;
}

// The impulse responses of rir_list, checked against the rate of the clean sentences (on: the list was given)
struct Reverb {
    bool on = false;
    std::vector<float> pcm;
    std::vector<int> len;
    int target = 0, early_taps = 0;
    std::vector<bp_rir_room> rooms;                              // rir_rooms: pcm is made from these by set_reverb
    int rate = 0;
};
void one_rate(const std::string &what, const std::vector<int> &clean_rates)
{
    for (size_t k = 0; k < clean_rates.size(); ++k)
        if (clean_rates[k] != clean_rates[0])
            die("bpmix: " + what + " needs clean sentences of one sample rate (sentence " + std::to_string(k) + " has " +
                std::to_string(clean_rates[k]) + " Hz, sentence 0 " + std::to_string(clean_rates[0]) + " Hz)");
}
// list: the responses of a rir_list; else n_rooms > 0: rooms drawn from the seed (checked here, made on the device by set_reverb)
Reverb read_reverb(const Params &P, const std::string &what, const std::string &list, int n_rooms, unsigned long long seed,
                   const std::vector<int> &clean_rates)
{
    Reverb r;
    if (list.empty() && n_rooms > 0) {
        one_rate("rir_rooms", clean_rates);
        const std::string err = bp::rir_draw(P.rir, seed, n_rooms, clean_rates[0], r.rooms, r.len);
        if (!err.empty()) die("bpmix: " + err);
        r.on = true; r.target = P.reverb_target; r.rate = clean_rates[0];
        r.early_taps = (int)((double)P.early_ms * clean_rates[0] / 1000.0 + 0.5);
        return r;
    }
    if (list.empty()) return r;
    std::vector<int> rates;
    const auto w = read_list(what, list, &rates);
    one_rate(what, clean_rates);
    for (size_t k = 0; k < w.size(); ++k) {
        if (rates[k] != clean_rates[0])
            die("bpmix: " + what + ": response " + std::to_string(k) + " has " + std::to_string(rates[k]) + " Hz, the clean sentences " +
                std::to_string(clean_rates[0]) + " Hz");
        if (w[k].size() > (size_t)BP_MIX_RIR_MAX_TAPS)
            die("bpmix: " + what + ": response " + std::to_string(k) + " has more than " + std::to_string(BP_MIX_RIR_MAX_TAPS) + " taps");
        for (float v : w[k])
            if (!std::isfinite(v)) die("bpmix: " + what + ": response " + std::to_string(k) + " has a tap that is not finite");
        r.pcm.insert(r.pcm.end(), w[k].begin(), w[k].end());
        r.len.push_back((int)w[k].size());
    }
    r.on = true; r.target = P.reverb_target;
    r.early_taps = (int)((double)P.early_ms * clean_rates[0] / 1000.0 + 0.5);
    return r;
}

// the derived entries of a corpus of n_clean sentences: sentence c with response bp_mix_reverb_pairs(seed)[c]
void set_reverb(bp_handle *h, const Params &P, const Reverb &r, unsigned long long seed, int n_clean)
{
    std::vector<float> made;
    if (!r.rooms.empty()) {
        const std::string err = bp::rir_generate(P.rir, P.device, r.rate, r.rooms, r.len, made);
        if (!err.empty()) die(err);
    }
    std::vector<int> pc(n_clean), pr(n_clean);
    for (int c = 0; c < n_clean; ++c) pc[c] = c;
    check(bp_mix_reverb_pairs(seed, n_clean, (int)r.len.size(), pr.data()));
    bp_mix_reverb mr;
    memset(&mr, 0, sizeof(mr));
    mr.n_rir = (int)r.len.size(); mr.rir_len = r.len.data(); mr.rir_pcm = r.rooms.empty() ? r.pcm.data() : made.data();
    mr.n_pair = n_clean; mr.pair_clean = pc.data(); mr.pair_rir = pr.data();
    mr.target = r.target; mr.early_taps = r.early_taps;
    check(bp_set_mix_reverb(h, &mr));
}

// Calls of at most `cap` rows (frames + n_mix (context-1)), consecutive mixtures of the plan: [first, last) per call.
std::vector<std::pair<int, int>> cut(const std::vector<bp_mixture> &plan, const Corpus &clean, int hop, int ctx, int cap, std::vector<int> *frames)
{
    std::vector<std::pair<int, int>> calls;
    int first = 0;
    long rows = 0, f = 0;
    frames->clear();
    for (int m = 0; m < (int)plan.size(); ++m) {
        const long T = (long)((clean.len[plan[m].clean] - 1) / hop + 2);
        if (T + ctx - 1 > cap) die("bpmix: clean sentence " + std::to_string(plan[m].clean) + " does not fit one chunk of traincache frames");
        if (rows + T + ctx - 1 > cap) { calls.push_back({first, m}); frames->push_back((int)f); first = m; rows = 0; f = 0; }
        rows += T + ctx - 1; f += T;
    }
    calls.push_back({first, (int)plan.size()});
    frames->push_back((int)f);
    return calls;
}

std::vector<bp_mixture> make_plan(unsigned long long seed, int n_clean, int per_clean, const Corpus &noise, const std::vector<float> &snr)
{
    std::vector<bp_mixture> plan((size_t)n_clean * per_clean);
    check(bp_mix_plan(seed, n_clean, per_clean, (int)noise.len.size(), noise.len.data(), (int)snr.size(), snr.data(), plan.data()));
    return plan;
}

bp_mix_corpus describe(const Params &P, int target, int ctx, int toff, const float *mean, const float *istd, const Corpus &c, const Corpus &n)
{
    bp_mix_corpus mc;
    memset(&mc, 0, sizeof(mc));
    mc.fea_dim = P.fea_dim; mc.context = ctx; mc.targ_offset = toff; mc.target = target; mc.lc_db = P.lc_db;
    mc.mean = mean; mc.inv_std = istd;
    mc.n_clean = (int)c.len.size(); mc.clean_len = c.len.data(); mc.clean_pcm = c.pcm.data();
    mc.n_noise = (int)n.len.size(); mc.noise_len = n.len.data(); mc.noise_pcm = n.pcm.data();
    return mc;
}

// norm_out: mean and inverse std of the noisy LPS of the epoch's training mixtures (bpfeat's format), on a one-layer handle
int norm_pass(const Params &P, const Corpus &clean, const Corpus &noise, std::vector<bp_mixture> plan, const Reverb &rv)
{
    const int D = P.fea_dim, hop = D - 1, cap = P.traincache ? P.traincache : BP_MAXCACHEFRAME;
    std::vector<int> frames;
    const auto calls = cut(plan, clean, hop, 1, cap, &frames);
    FILE *fn = fopen(P.norm_out.c_str(), "wt");
    if (!fn) die("can not open norm file: " + P.norm_out);
    bp_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.gpu_used = 1; cfg.numlayers = 2; cfg.layersizes[0] = D; cfg.layersizes[1] = D; cfg.bunchsize = 256; cfg.device = P.device;
    cfg.max_chunk_frames = cap;
    std::vector<float> W((size_t)D * D, 0.f), B(D, 0.f), mean(D, 0.f), istd(D, 1.f);
    float *w[BP_MAXLAYER] = {0}, *b[BP_MAXLAYER] = {0};
    w[1] = W.data(); b[1] = B.data();
    bp_handle *h = nullptr;
    check(bp_create(&cfg, w, b, &h));
    const bp_mix_corpus mc = describe(P, BP_MIX_LPS, 1, 0, mean.data(), istd.data(), clean, noise);
    check(bp_set_mix_corpus(h, &mc));
    if (rv.on) {
        set_reverb(h, P, rv, P.seed, (int)clean.len.size());
        for (bp_mixture &m : plan) m.clean += (int)clean.len.size();
    }
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
    fprintf(fn, "<mean>\n");
    for (int j = 0; j < D; ++j) fprintf(fn, "%.9g\n", sum[j] / total);
    fprintf(fn, "<inverse std>\n");
    for (int j = 0; j < D; ++j) {
        const double m = sum[j] / total, var = sq[j] / total - m * m;
        fprintf(fn, "%.9g\n", var > 0.0 ? 1.0 / sqrt(var) : 1.0);
    }
    fclose(fn);
    printf("bpmix: norm file of %zu noisy frames of %zu mixtures -> %s\n", total, plan.size(), P.norm_out.c_str());
    return 1;
}

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

}  // namespace

int main(int argc, char **argv)
{
    const double t_start = (double)time(NULL);
    const Params P = parse(argc, argv);
    const int D = P.fea_dim, n_fft = 2 * (D - 1);
    if (D < 33 || D > 1025 || (n_fft & (n_fft - 1))) die("bpmix: fea_dim must make 2*(fea_dim-1) a power of two from 64 to 2048");
    if (P.snr.empty()) die("bpmix: snr_list is empty");
    const int hop = D - 1;
    // every list and WAV is read and checked before the device is used
    std::vector<int> clean_rates, cv_rates;
    const Corpus clean = flatten(read_list("clean_list", P.clean_list, &clean_rates));
    const Corpus noise = flatten(read_list("noise_list", P.noise_list));
    for (int64_t n : noise.len)
        if (n >= ((int64_t)1 << 32)) die("bpmix: a noise recording has 2^32 samples or more");
    std::vector<bp_mixture> plan = make_plan(P.seed, (int)clean.len.size(), P.mix_per_clean, noise, P.snr);
    if (P.rir.rooms && !P.rir_list.empty()) die("bpmix: rir_rooms and rir_list exclude each other");
    if ((P.rir.cv_rooms || P.rir.rooms) && !P.cv_rir_list.empty()) die("bpmix: rir_rooms / cv_rir_rooms and cv_rir_list exclude each other");
    if ((P.rir.any || P.rir.cv_rooms) && !P.rir.rooms) die("bpmix: the rir_* keys need rir_rooms");
    const Reverb rv = read_reverb(P, "rir_list", P.rir_list, P.rir.rooms, P.seed, clean_rates);
    if (!P.rir.rooms_out.empty()) {
        const std::string err = bp::rir_write_rooms(P.rir.rooms_out, rv.rooms);
        if (!err.empty()) die(err);
    }
    if (!P.norm_out.empty()) return norm_pass(P, clean, noise, plan, rv);

    const int L = P.numlayers, ctx = P.fea_context, toff = P.targ_offset;
    if (L < 2 || P.layersizes[L - 1] < 1) die("bpmix: numlayers / layersizes: need 2.." + std::to_string(BP_MAXLAYER - 1) + " layer sizes");
    if (P.outwts_file.empty() || P.log_file.empty() || P.norm_file.empty()) die("bpmix: need norm_file, outwts_file and log_file");
    if (P.traincache < 1 || P.bunchsize < 1) die("bpmix: need traincache and bunchsize");
    if (toff >= ctx) die("bpmix: targ_offset must be below fea_context");
    const int parts = P.target == BP_MIX_LPS_IRM || P.target == BP_MIX_LPS_IBM ? 2 : 1;
    if (P.layersizes[L - 1] != parts * D) die("bpmix: layersizes[last] must be " + std::to_string(parts * D) + " for this target");
    if (P.layersizes[0] != ctx * D && P.layersizes[0] != (ctx + 1) * D) die("bpmix: layersizes[0] must be fea_context*fea_dim (+ fea_dim with NAT)");
    const Corpus cv_clean = flatten(read_list("cv_clean_list", P.cv_clean_list, &cv_rates));
    const Corpus cv_noise = P.cv_noise_list.empty() ? noise : flatten(read_list("cv_noise_list", P.cv_noise_list));
    std::vector<bp_mixture> cv_plan = make_plan(P.cv_seed, (int)cv_clean.len.size(), 1, cv_noise, P.snr);
    const Reverb cv_rv = read_reverb(P, P.cv_rir_list.empty() ? "rir_list" : "cv_rir_list", P.cv_rir_list.empty() ? P.rir_list : P.cv_rir_list,
                                     P.rir.rooms ? (P.rir.cv_rooms ? P.rir.cv_rooms : P.rir.rooms) : 0, P.cv_seed, cv_rates);
    std::vector<int> frames, cv_frames;
    const auto calls = cut(plan, clean, hop, ctx, P.traincache, &frames);
    const auto cv_calls = cut(cv_plan, cv_clean, hop, ctx, P.traincache, &cv_frames);
    if (rv.on) for (bp_mixture &m : plan) m.clean += (int)clean.len.size();          // (the derived entry of sentence c: n_clean + c)
    if (cv_rv.on) for (bp_mixture &m : cv_plan) m.clean += (int)cv_clean.len.size();
    std::vector<float> mean, istd;
    read_norm(P.norm_file, D, mean, istd);

    FILE *log = fopen(P.log_file.c_str(), "wt");
    if (!log) die("can not open output log file: " + P.log_file);
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

    std::vector<std::vector<float>> Wv(L), Bv(L);
    float *weights[BP_MAXLAYER] = {0}, *bias[BP_MAXLAYER] = {0};
    for (int i = 1; i < L; ++i) {
        Wv[i].assign((size_t)P.layersizes[i] * P.layersizes[i - 1], 0.f); Bv[i].assign(P.layersizes[i], 0.f);
        weights[i] = Wv[i].data(); bias[i] = Bv[i].data();
    }
    srand48((long)P.seed);
    if (P.initwts_file.empty()) {
        fprintf(log, "Getting Randemed initial weights...\n");
        bp::random_weights(L, P.layersizes, weights, bias, P.wmin, P.wmax, P.bmin, P.bmax);
        fprintf(log, "Randemed initial weights getted.\n");
    } else {
        FILE *fi = fopen(P.initwts_file.c_str(), "rb");
        if (!fi) { fprintf(log, "can not open initial weights file: %s\n", P.initwts_file.c_str()); exit(0); }
        fprintf(log, "Loading Init weight file...\n");
        const std::string err = bp::read_weights(fi, L, P.layersizes, weights, bias);
        fclose(fi);
        if (!err.empty()) { fprintf(log, "%s\n", err.c_str()); exit(0); }
        fprintf(log, "Init weight file loaded.\n");
    }
    fflush(log);

    bp_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.gpu_used = 1; cfg.numlayers = L;
    for (int i = 0; i < L; ++i) cfg.layersizes[i] = P.layersizes[i];
    cfg.bunchsize = P.bunchsize; cfg.lrate = P.lrate; cfg.momentum = P.momentum; cfg.weightcost = P.weightcost;
    cfg.dropoutflag = P.dropoutflag; cfg.visible_omit = P.visible_omit; cfg.hid_omit = P.hid_omit;
    cfg.activation = P.activation; cfg.momentum_rule = P.momentum_rule; cfg.seed = P.dropout_seed; cfg.compute_dtype = P.compute_dtype;
    cfg.max_chunk_frames = P.traincache; cfg.device = P.device;
    bp_handle *h = nullptr;
    check(bp_create(&cfg, weights, bias, &h));
    check(bp_set_output(h, P.output_act, P.output_linear_dims, P.output_loss));
    printf("Created net with %d layers, bunchsize %d.\n", L, P.bunchsize);
    const bp_mix_corpus mc = describe(P, P.target, ctx, toff, mean.data(), istd.data(), clean, noise);
    check(bp_set_mix_corpus(h, &mc));
    if (rv.on) {
        set_reverb(h, P, rv, P.seed, (int)clean.len.size());
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
    check(bp_get_weights(h, weights, bias));
    clock_gettime(CLOCK_MONOTONIC, &ts1);
    {
        const double dt = (double)(ts1.tv_sec - ts0.tv_sec) + 1e-9 * (double)(ts1.tv_nsec - ts0.tv_nsec);
        fprintf(log, "Training pass: %ld samples in %.3f s (%.0f frames/s, mixing + GPU).\n", total, dt, dt > 0 ? total / dt : 0.0);
    }
    fprintf(log, "Saving weights to file...\n");
    bp::write_weights(fp_out, L, P.layersizes, weights, bias);
    fclose(fp_out);
    fprintf(log, "Saving over.\n");
    printf("finish to write weights\n\n");

    printf("begin to CV\n");
    fprintf(log, "Starting CV.\n");
    const bp_mix_corpus cvc = describe(P, P.target, ctx, toff, mean.data(), istd.data(), cv_clean, cv_noise);
    check(bp_set_mix_corpus(h, &cvc));
    if (cv_rv.on) set_reverb(h, P, cv_rv, P.cv_seed, (int)cv_clean.len.size());
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
