// List files, WAV lists and the mixing corpus of bpmix and bpeval.  `who` is the tool's name and `what` the key
// or kind of list, as the messages quote them.  Everything here except set_reverb runs before the device is used; errors end
// the run through bp::fail (keys.h).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/bp_c_api.h"
#include "keys.h"
#include "rir_keys.h"
#include "wav_io.h"

namespace bp {

inline std::string trim(std::string s)
{
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ' || s.back() == '\t')) s.pop_back();
    size_t i = 0;
    while (i < s.size() && (s[i] == ' ' || s[i] == '\t')) ++i;
    return s.substr(i);
}

// the analysis sizes of bp_wave.hip: 2*(fea_dim-1) a power of two from 64 to 2048
inline bool fea_dim_ok(int D)
{
    const int n_fft = 2 * (D - 1);
    return D >= 33 && D <= 1025 && !(n_fft & (n_fft - 1));
}

// the lines of a list file that are not blank, trimmed; at least one
inline std::vector<std::string> read_lines(const std::string &who, const std::string &what, const std::string &list)
{
    if (list.empty()) fail(who + ": " + what + " is not given");
    FILE *fl = fopen(list.c_str(), "rt");
    if (!fl) fail("can not open " + what + ": " + list);
    std::vector<std::string> out;
    char line[8192];
    while (fgets(line, sizeof(line), fl)) {
        const std::string t = trim(line);
        if (!t.empty()) out.push_back(t);
    }
    fclose(fl);
    if (out.empty()) fail(who + ": " + list + " lists no wav file");
    return out;
}

// two paths per line; needs: what a line must hold, as its message says it
inline void read_pairs(const std::string &who, const std::string &what, const std::string &title, const std::string &needs,
                       const std::string &list, std::vector<std::string> &first, std::vector<std::string> &second)
{
    for (const std::string &t : read_lines(who, what, list)) {
        const size_t sp = t.find_first_of(" \t");
        if (sp == std::string::npos) fail(title + " " + list + ": line \"" + t + "\" needs " + needs);
        first.push_back(t.substr(0, sp)); second.push_back(trim(t.substr(sp)));
    }
}

// one WAV, not empty.  *rate != 0 demands that rate; *rate is the file's afterwards
inline std::vector<float> read_one(const std::string &who, const std::string &path, int *rate)
{
    std::vector<float> w;
    int sr = 0;
    const std::string err = read_wav(path, w, sr);
    if (!err.empty()) fail(err);
    if (w.empty()) fail(path + ": no samples");
    if (*rate && sr != *rate) fail(who + ": " + path + " has " + std::to_string(sr) + " Hz, the others " + std::to_string(*rate) + " Hz");
    *rate = sr;
    return w;
}

// ---- rate=R: files of other rates converted on the device as they are loaded
// a file of f Hz can be brought to R Hz (and back): checked where the file is read, before the device is used
inline void check_convertible(const std::string &who, const std::string &path, int f, int R)
{
    int p = 0, q = 0;
    if (f != R && bp_resample_ratio(f, R, &p, &q) != 0)
        fail(who + ": " + path + " has " + std::to_string(f) + " Hz and rate=" + std::to_string(R) + " cannot convert it (" + bp_last_error() + ")");
}
// The recordings whose rate is not `to` become recordings at `to`: one bp_resample_waves call and one line on stdout per
// distinct rate, in the order the rates first appear; the float samples go on as they come, nothing is re-quantised.
// from != 0: the other direction -- every recording is at `from` and goes to its rates[k] (bpenhance, on the way out).
inline void convert_rates(const std::string &who, const std::string &what, int device, int to, std::vector<std::vector<float>> &waves,
                          const std::vector<int> &rates, int from = 0)
{
    std::vector<int> todo;
    for (int f : rates)
        if (f != (from ? from : to) && std::find(todo.begin(), todo.end(), f) == todo.end()) todo.push_back(f);
    for (int f : todo) {
        const int r_in = from ? from : f, r_out = from ? f : to;
        int p = 0, q = 0;
        check(bp_resample_ratio(r_in, r_out, &p, &q));
        std::vector<float> pcm, out;
        std::vector<int> lens;
        std::vector<size_t> idx;
        size_t n_out = 0;
        for (size_t k = 0; k < waves.size(); ++k) {
            if (rates[k] != f) continue;
            if (waves[k].size() > (size_t)INT32_MAX) fail(who + ": " + what + ": recording " + std::to_string(k) + " is too long to convert");
            int64_t no = 0;
            check(bp_resample_len((int64_t)waves[k].size(), p, q, &no));
            idx.push_back(k); lens.push_back((int)waves[k].size()); n_out += (size_t)no;
            pcm.insert(pcm.end(), waves[k].begin(), waves[k].end());
        }
        out.resize(n_out);
        check(bp_resample_waves(device, r_in, r_out, nullptr, (int)idx.size(), lens.data(), pcm.data(), out.data()));
        size_t at = 0;
        for (size_t k : idx) {
            int64_t no = 0;
            check(bp_resample_len((int64_t)waves[k].size(), p, q, &no));
            waves[k].assign(out.begin() + at, out.begin() + at + no);
            at += (size_t)no;
        }
        printf("%s: %s: %zu recording%s converted from %d Hz to %d Hz (%zu samples)\n", who.c_str(), what.c_str(), idx.size(),
               idx.size() == 1 ? "" : "s", r_in, r_out, n_out);
    }
}

// one WAV per line.  rates: the rate of every file, for the caller to judge (bpmix); one_rate: the rate every file must have,
// 0 until the first one sets it, carried from list to list (bpeval).  to_rate != 0 (rate=R): a file may have any rate that can be
// converted; the list comes back at to_rate, and so do *rates and *one_rate
inline std::vector<std::vector<float>> read_wav_list(const std::string &who, const std::string &what, const std::string &list,
                                                     std::vector<int> *rates = nullptr, int *one_rate = nullptr, int to_rate = 0, int device = 0)
{
    std::vector<std::vector<float>> waves;
    std::vector<int> file_rates;
    for (const std::string &p : read_lines(who, what, list)) {
        int sr = one_rate && !to_rate ? *one_rate : 0;
        waves.push_back(read_one(who, p, &sr));
        if (to_rate) { check_convertible(who, p, sr, to_rate); file_rates.push_back(sr); sr = to_rate; }
        if (one_rate) *one_rate = sr;
        if (rates) rates->push_back(sr);
    }
    if (to_rate) convert_rates(who, what, device, to_rate, waves, file_rates);
    return waves;
}

// ---- the mixing corpus: recordings back to back
struct Corpus {
    std::vector<float> pcm;
    std::vector<int64_t> len;
};
inline Corpus flatten(const std::vector<std::vector<float>> &w)
{
    Corpus c;
    for (const auto &x : w) { c.pcm.insert(c.pcm.end(), x.begin(), x.end()); c.len.push_back((int64_t)x.size()); }
    return c;
}

inline void check_fea_dim(const std::string &who, int D)
{
    if (!fea_dim_ok(D)) fail(who + ": fea_dim must make 2*(fea_dim-1) a power of two from 64 to 2048");
}
inline void check_noise(const std::string &who, const Corpus &noise)
{
    for (int64_t n : noise.len)
        if (n >= ((int64_t)1 << 32)) fail(who + ": a noise recording has 2^32 samples or more");
}
// rir_rooms stands in place of the lists; the other rir_* keys only go with it.  hint: appended to the last message
inline void check_rir_keys(const std::string &who, const RirKeys &K, const std::string &rir_list, const std::string &cv_rir_list, const char *hint)
{
    if (K.rooms && !rir_list.empty()) fail(who + ": rir_rooms and rir_list exclude each other");
    if ((K.cv_rooms || K.rooms) && !cv_rir_list.empty()) fail(who + ": rir_rooms / cv_rir_rooms and cv_rir_list exclude each other");
    if ((K.any || K.cv_rooms) && !K.rooms) fail(who + ": the rir_* keys need rir_rooms" + hint);
}

inline std::vector<bp_mixture> make_plan(unsigned long long seed, int n_clean, int per_clean, const Corpus &noise, const std::vector<float> &snr)
{
    std::vector<bp_mixture> plan((size_t)n_clean * per_clean);
    check(bp_mix_plan(seed, n_clean, per_clean, (int)noise.len.size(), noise.len.data(), (int)snr.size(), snr.data(), plan.data()));
    return plan;
}

// Calls of at most `cap` rows (frames + n_mix (context-1)), consecutive mixtures of the plan: [first, last) per call.
// frames: the frames of every call, where the caller wants them
inline std::vector<std::pair<int, int>> cut(const std::string &who, const std::vector<bp_mixture> &plan, const Corpus &clean, int hop, int ctx, int cap,
                                            std::vector<int> *frames = nullptr)
{
    std::vector<std::pair<int, int>> calls;
    int first = 0;
    long rows = 0, f = 0;
    if (frames) frames->clear();
    for (int m = 0; m < (int)plan.size(); ++m) {
        const long T = (long)((clean.len[plan[m].clean] - 1) / hop + 2);
        if (T + ctx - 1 > cap) fail(who + ": clean sentence " + std::to_string(plan[m].clean) + " does not fit one chunk of traincache frames");
        if (rows + T + ctx - 1 > cap) {
            calls.push_back({first, m});
            if (frames) frames->push_back((int)f);
            first = m; rows = 0; f = 0;
        }
        rows += T + ctx - 1; f += T;
    }
    calls.push_back({first, (int)plan.size()});
    if (frames) frames->push_back((int)f);
    return calls;
}

inline bp_mix_corpus describe(int fea_dim, int ctx, int toff, int target, float lc_db, const float *mean, const float *istd, const Corpus &c,
                              const Corpus &n)
{
    bp_mix_corpus mc;
    memset(&mc, 0, sizeof(mc));
    mc.fea_dim = fea_dim; mc.context = ctx; mc.targ_offset = toff; mc.target = target; mc.lc_db = lc_db;
    mc.mean = mean; mc.inv_std = istd;
    mc.n_clean = (int)c.len.size(); mc.clean_len = c.len.data(); mc.clean_pcm = c.pcm.data();
    mc.n_noise = (int)n.len.size(); mc.noise_len = n.len.data(); mc.noise_pcm = n.pcm.data();
    return mc;
}

// ---- reverberation: the responses of a rir_list (pcm), or rooms drawn from the seed (made on the device by set_reverb)
struct Reverb {
    bool on = false;
    std::vector<float> pcm;
    std::vector<int> len;
    int target = 0, early_taps = 0;
    std::vector<bp_rir_room> rooms;
    int rate = 0;
};
inline int early_taps(float early_ms, int rate) { return (int)((double)early_ms * rate / 1000.0 + 0.5); }

// the derived entries of a corpus of n_clean sentences: sentence c with response bp_mix_reverb_pairs(seed)[c]
inline void set_reverb(bp_handle *h, const RirKeys &K, int device, const Reverb &r, unsigned long long seed, int n_clean)
{
    std::vector<float> made;
    if (!r.rooms.empty()) {
        const std::string err = rir_generate(K, device, r.rate, r.rooms, r.len, made);
        if (!err.empty()) fail(err);
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
// ... which the plan then addresses: entry n_clean + c in place of sentence c
inline void address_reverberant(std::vector<bp_mixture> &plan, const Reverb &r, int n_clean)
{
    if (r.on) for (bp_mixture &m : plan) m.clean += n_clean;
}

}  // namespace bp
