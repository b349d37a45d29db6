// bpenhance.cpp -- waveform enhancement: noisy WAV in, enhanced WAV out, on the MI355X through bp_enhance_waves (analysis,
// the forward of bpforward, resynthesis, overlap-add; include/bp_c_api.h).
//
//   bpenhance norm_file=x.norm initwts_file=mlp.N.wts layersizes=1548,2048,2048,2048,129 fea_dim=129 fea_context=11
//             targ_offset=5 (wav_list=<"in.wav out.wav" per line> | in_wav=noisy.wav out_wav=enh.wav)
//             [wave_target=lps|mask] [out_col=0] [dropoutflag=1 visible_omit=0.1 hid_omit=0.2] [bunchsize=1024]
//             [traincache=102400] [activation=relu|sigmoid] [device=0] [compute=fp32|bf16]
//             [output_act=linear|sigmoid output_linear_dims=<n> output_loss=xent|mse]   (as the net was trained, bptrain.cpp)
//             [stream_block=<samples> [stream_chan=<n>]] [forward=default|rowinv]
//   bpenhance method=logmmse fea_dim=129 (wav_list=... | in_wav=... out_wav=...) [device=0] [lm_alpha=0.98] [lm_mu=0.98]
//             [lm_eta=0.15] [lm_xi_min_db=-25] [lm_gamma_max=40] [lm_init_frames=6] [lm_stream_block=<samples> [lm_stream_chan=<n>]]
//
// As many sentences go into one call as fit traincache rows (frames + context-1 replicated edge rows per sentence).  The
// output is PCM16 at the input's sample rate, rounded to nearest and clipped.  Every input is read and checked before the
// device is used.  With stream_block the files go through a streaming session instead (bp_stream_push): they
// are dealt to stream_chan channels (file s to channel s mod stream_chan) and pushed stream_block samples at a time, the last
// block of a file with its end flag -- the way a live feed would arrive; the output files hold the bytes of a run without
// stream_block that enhances one sentence per call.  forward=rowinv selects the row-invariant forward (bp_set_forward,
// INTEGRATION.md 1i; fp32): a sentence's bytes then do not depend on what else went into its call, and a streaming session packs
// its channels.  method=logmmse is the classic baseline instead of a net (bp_logmmse_waves,
// INTEGRATION.md 1h): no weights, no norm file; it takes only the keys of its line above, and the lm_ keys only go with it.
// With lm_stream_block the files go through a log-MMSE stream (bp_lmstream_push) by the rules of stream_block:
// file s to channel s mod lm_stream_chan, lm_stream_block samples per push, the end flag on a file's last block; the output
// files hold the bytes of a run without the key.
// Errors: message + exit(0), success: return 1 (reference convention).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../../include/BP_GPU.h"
#include "wav_io.h"
#include "wts_io.h"

static std::string trim(std::string s)
{
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ' || s.back() == '\t')) s.pop_back();
    size_t i = 0;
    while (i < s.size() && (s[i] == ' ' || s[i] == '\t')) ++i;
    return s.substr(i);
}

// the input and output files of wav_list, or the one pair
static void read_wav_list(const std::string &list, const std::string &in_wav, const std::string &out_wav, std::vector<std::string> &ins,
                          std::vector<std::string> &outs)
{
    if (list.empty()) { ins.push_back(in_wav); outs.push_back(out_wav); return; }
    FILE *fl = fopen(list.c_str(), "rt");
    if (!fl) { printf("can not open wav list: %s\n", list.c_str()); exit(0); }
    char line[8192];
    while (fgets(line, sizeof(line), fl)) {
        const std::string t = trim(line);
        if (t.empty()) continue;
        const size_t sp = t.find_first_of(" \t");
        if (sp == std::string::npos) { printf("wav list %s: line \"%s\" needs an input and an output file\n", list.c_str(), t.c_str()); exit(0); }
        ins.push_back(t.substr(0, sp)); outs.push_back(trim(t.substr(sp)));
    }
    fclose(fl);
    if (ins.empty()) { printf("bpenhance: %s lists no wav file\n", list.c_str()); exit(0); }
}

// method=logmmse: every file through bp_logmmse_waves, as many sentences per call as stay below MAXCACHEFRAME frames
static int logmmse_mode(int fea_dim, int device, const bp_logmmse_params &lm, const std::vector<std::string> &ins, const std::vector<std::string> &outs)
{
    const int ns = (int)ins.size(), hop = fea_dim - 1;
    std::vector<std::vector<float>> waves(ns);
    std::vector<int> rates(ns);
    for (int s = 0; s < ns; ++s) {
        const std::string err = bp::read_wav(ins[s], waves[s], rates[s]);
        if (!err.empty()) { printf("%s\n", err.c_str()); exit(0); }
        if (waves[s].empty()) { printf("%s: no samples\n", ins[s].c_str()); exit(0); }
        if (waves[s].size() > (size_t)1 << 30) { printf("%s: too long\n", ins[s].c_str()); exit(0); }
    }
    std::vector<float> pcm, out;
    std::vector<int> lens;
    size_t samples = 0;
    for (int s0 = 0; s0 < ns;) {
        int s1 = s0;
        size_t frames = 0;
        pcm.clear(); lens.clear();
        while (s1 < ns) {
            const size_t T = (waves[s1].size() - 1) / hop + 2;
            if (s1 > s0 && frames + T > (size_t)MAXCACHEFRAME) break;
            frames += T;
            pcm.insert(pcm.end(), waves[s1].begin(), waves[s1].end());
            lens.push_back((int)waves[s1].size());
            ++s1;
        }
        out.resize(pcm.size());
        if (bp_logmmse_waves(device, fea_dim, &lm, s1 - s0, lens.data(), pcm.data(), out.data(), nullptr, nullptr) != 0) { printf("%s\n", bp_last_error()); exit(0); }
        size_t off = 0;
        for (int s = s0; s < s1; ++s) {
            const std::string e = bp::write_wav(outs[s], &out[off], waves[s].size(), rates[s]);
            if (!e.empty()) { printf("%s\n", e.c_str()); exit(0); }
            off += waves[s].size();
        }
        samples += pcm.size();
        s0 = s1;
    }
    printf("bpenhance: %zu samples of %d sentences enhanced (logmmse)\n", samples, ns);
    return 1;
}

// A streaming run of either kind (stream_block, lm_stream_block): channel c plays files c, c + chan, ... one after the other,
// `block` samples per push, the last block of a file with its end flag.  push is bp_stream_push or bp_lmstream_push, st its open
// stream; out_cap: the samples one push can return.  Returns the samples pushed; enh[s]: what came back for file s.
template <class S>
static size_t play_files(S *st, int (*push)(S *, const int *, const float *, const unsigned char *, int *, float *, size_t), int chan, int block,
                         const std::vector<std::string> &ins, const std::vector<std::vector<float>> &waves, size_t out_cap,
                         std::vector<std::vector<float>> &enh)
{
    const int ns = (int)waves.size();
    std::vector<int> file(chan), n_in(chan), n_out(chan);
    std::vector<size_t> pos(chan, 0);
    std::vector<unsigned char> end(chan);
    std::vector<float> pcm, out(out_cap);
    size_t samples = 0;
    enh.assign(ns, std::vector<float>());
    for (int c = 0; c < chan; ++c) file[c] = c;
    for (;;) {
        pcm.clear();
        bool any = false;
        for (int c = 0; c < chan; ++c) {
            n_in[c] = 0; end[c] = 0;
            if (file[c] >= ns) continue;
            const std::vector<float> &w = waves[file[c]];
            n_in[c] = (int)std::min((size_t)block, w.size() - pos[c]);
            end[c] = pos[c] + n_in[c] == w.size();
            pcm.insert(pcm.end(), w.begin() + pos[c], w.begin() + pos[c] + n_in[c]);
            any = true;
        }
        if (!any) break;
        if (push(st, n_in.data(), pcm.data(), end.data(), n_out.data(), out.data(), out.size()) != 0) { printf("%s\n", bp_last_error()); exit(0); }
        size_t off = 0;
        for (int c = 0; c < chan; ++c) {
            if (file[c] >= ns) continue;
            enh[file[c]].insert(enh[file[c]].end(), out.begin() + off, out.begin() + off + n_out[c]);
            off += n_out[c];
            pos[c] += n_in[c];
            if (end[c]) { file[c] += chan; pos[c] = 0; }
        }
        samples += pcm.size();
    }
    for (int s = 0; s < ns; ++s)
        if (enh[s].size() != waves[s].size()) { printf("%s: the stream returned %zu of %zu samples\n", ins[s].c_str(), enh[s].size(), waves[s].size()); exit(0); }
    return samples;
}

// method=logmmse lm_stream_block=...: the files through a log-MMSE stream
static int logmmse_stream_mode(int fea_dim, int device, const bp_logmmse_params &lm, int block, int chan, const std::vector<std::string> &ins,
                               const std::vector<std::string> &outs)
{
    const int ns = (int)ins.size(), hop = fea_dim - 1;
    std::vector<std::vector<float>> waves(ns), enh;
    std::vector<int> rates(ns);
    for (int s = 0; s < ns; ++s) {
        const std::string err = bp::read_wav(ins[s], waves[s], rates[s]);
        if (!err.empty()) { printf("%s\n", err.c_str()); exit(0); }
        if (waves[s].empty()) { printf("%s: no samples\n", ins[s].c_str()); exit(0); }
    }
    bp_lmstream *st = nullptr;
    if (bp_lmstream_open(device, fea_dim, &lm, chan, block * chan, &st) != 0) { printf("%s\n", bp_last_error()); exit(0); }
    // a push returns what arrived plus what waited for the noise start or for the end of the sentence
    const size_t samples = play_files(st, bp_lmstream_push, chan, block, ins, waves, (size_t)chan * ((size_t)block + ((size_t)lm.init_frames + 1) * hop), enh);
    bp_lmstream_close(st);
    for (int s = 0; s < ns; ++s) {
        const std::string e = bp::write_wav(outs[s], enh[s].data(), waves[s].size(), rates[s]);
        if (!e.empty()) { printf("%s\n", e.c_str()); exit(0); }
    }
    printf("bpenhance: %zu samples of %d sentences enhanced (logmmse, streamed)\n", samples, ns);
    return 1;
}

int main(int argc, char **argv)
{
    std::string norm_file, wts_file, list, in_wav, out_wav;
    bool logmmse = false;
    std::vector<std::string> given;
    bp_logmmse_params lm;
    bp_logmmse_defaults(&lm);
    int fea_dim = 0, ctx = 1, toff = 0, dropoutflag = 0, bunch = 1024, cache = 102400, L = 0, ls[MAXLAYER] = {0};
    int activation = 0, device = 0, compute = 0, out_act = 0, out_lin = 0, out_loss = 0, target = BP_WAVE_LPS, out_col = 0;
    int stream_block = 0, stream_chan = 1, forward = BP_FORWARD_DEFAULT, lm_block = 0, lm_chan = 1;
    bool lm_chan_given = false;
    float vis = 0.f, hid = 0.f;
    for (int i = 1; i < argc; ++i) {
        char *eq = strchr(argv[i], '=');
        if (!eq) { printf("Arg: %s  Format Error\n", argv[i]); exit(0); }
        const std::string k(argv[i], eq - argv[i]), v(eq + 1);
        given.push_back(k);
        if (k == "method") {
            if (v == "net") logmmse = false; else if (v == "logmmse") logmmse = true;
            else { printf("method: %s is not net or logmmse\n", v.c_str()); exit(0); }
        } else if (k == "lm_stream_block" || k == "lm_stream_chan") {
            char *end = nullptr;
            const long n = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || n < 1 || n > (1 << 24)) { printf("%s: %s is not a count >= 1\n", k.c_str(), v.c_str()); exit(0); }
            if (k == "lm_stream_block") lm_block = (int)n; else { lm_chan = (int)n; lm_chan_given = true; }
        } else if (k.compare(0, 3, "lm_") == 0) {
            char *end = nullptr;
            const double d = strtod(v.c_str(), &end);
            if (v.empty() || *end) { printf("%s: %s is not a number\n", k.c_str(), v.c_str()); exit(0); }
            if (k == "lm_alpha") lm.alpha = d; else if (k == "lm_mu") lm.mu = d; else if (k == "lm_eta") lm.eta = d;
            else if (k == "lm_xi_min_db") lm.xi_min_db = d; else if (k == "lm_gamma_max") lm.gamma_max = d;
            else if (k == "lm_init_frames") {
                if (!(d >= -1e9 && d <= 1e9) || d != (double)(int)d) { printf("%s: %s is not a count\n", k.c_str(), v.c_str()); exit(0); }
                lm.init_frames = (int)d;
            }
            else { printf("bpenhance: unknown key %s\n", k.c_str()); exit(0); }
        }
        else if (k == "norm_file") norm_file = v; else if (k == "initwts_file") wts_file = v;
        else if (k == "wav_list") list = v; else if (k == "in_wav") in_wav = v; else if (k == "out_wav") out_wav = v;
        else if (k == "fea_dim") fea_dim = atoi(v.c_str()); else if (k == "fea_context") ctx = atoi(v.c_str());
        else if (k == "targ_offset") toff = atoi(v.c_str()); else if (k == "dropoutflag") dropoutflag = atoi(v.c_str());
        else if (k == "visible_omit") vis = (float)atof(v.c_str()); else if (k == "hid_omit") hid = (float)atof(v.c_str());
        else if (k == "bunchsize") bunch = atoi(v.c_str()); else if (k == "traincache") cache = atoi(v.c_str());
        else if (k == "activation") activation = v == "sigmoid" ? 1 : 0; else if (k == "device") device = atoi(v.c_str());
        else if (k == "compute") compute = v == "bf16" ? 1 : 0;
        else if (k == "out_col") out_col = atoi(v.c_str());
        else if (k == "stream_block" || k == "stream_chan") {
            char *end = nullptr;
            const long n = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || n < 1 || n > (1 << 24)) { printf("%s: %s is not a count >= 1\n", k.c_str(), v.c_str()); exit(0); }
            (k == "stream_block" ? stream_block : stream_chan) = (int)n;
        }
        else if (k == "forward") {
            if (v == "default") forward = BP_FORWARD_DEFAULT; else if (v == "rowinv") forward = BP_FORWARD_ROWINV;
            else { printf("forward: %s is not default or rowinv\n", v.c_str()); exit(0); }
        }
        else if (k == "wave_target") {
            if (v == "lps") target = BP_WAVE_LPS; else if (v == "mask") target = BP_WAVE_MASK;
            else { printf("wave_target: %s is not lps or mask\n", v.c_str()); exit(0); }
        }
        // output layer (.wts files do not record it): the keys and checks of bptrain
        else if (k == "output_act") {
            if (v == "linear") out_act = 0; else if (v == "sigmoid") out_act = 1;
            else { printf("output_act: %s is not linear or sigmoid\n", v.c_str()); exit(0); }
        } else if (k == "output_linear_dims") {
            char *end = nullptr;
            const long n = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || n < 0 || n > 1000000) { printf("output_linear_dims: %s is not a column count\n", v.c_str()); exit(0); }
            out_lin = (int)n;
        } else if (k == "output_loss") {
            if (v == "xent") out_loss = 0; else if (v == "mse") out_loss = 1;
            else { printf("output_loss: %s is not xent or mse\n", v.c_str()); exit(0); }
        }
        else if (k == "layersizes") {
            size_t pos = 0;
            while (L < MAXLAYER) {
                const size_t c = v.find(',', pos);
                ls[L++] = atoi(v.substr(pos, c == std::string::npos ? c : c - pos).c_str());
                if (c == std::string::npos) break;
                pos = c + 1;
            }
        }
        else { printf("bpenhance: unknown key %s\n", k.c_str()); exit(0); }
    }
    for (const std::string &k : given) {
        const bool lm_key = k.compare(0, 3, "lm_") == 0;
        if (!logmmse && lm_key) { printf("bpenhance: %s needs method=logmmse\n", k.c_str()); exit(0); }
        if (logmmse && !lm_key && k != "method" && k != "fea_dim" && k != "device" && k != "wav_list" && k != "in_wav" && k != "out_wav") {
            printf("bpenhance: method=logmmse takes no %s (only fea_dim, device, wav_list or in_wav and out_wav, and the lm_ keys, lm_stream_block and lm_stream_chan among them)\n", k.c_str());
            exit(0);
        }
    }
    if (logmmse) {
        if (list.empty() == (in_wav.empty() || out_wav.empty())) { printf("bpenhance: need wav_list, or in_wav and out_wav\n"); exit(0); }
        const int nf = 2 * (fea_dim - 1);
        if (fea_dim < 33 || fea_dim > 1025 || (nf & (nf - 1))) { printf("bpenhance: 2*(fea_dim-1) must be a power of two from 64 to 2048\n"); exit(0); }
        if (lm_chan_given && lm_block < 1) { printf("bpenhance: lm_stream_chan needs lm_stream_block\n"); exit(0); }
        if (lm_block > 0 && ((long)lm_block * lm_chan > (1L << 28) || lm_chan > (1 << 16))) { printf("bpenhance: lm_stream_block * lm_stream_chan is too large\n"); exit(0); }
        std::vector<std::string> li, lo;
        read_wav_list(list, in_wav, out_wav, li, lo);
        if (lm_block > 0) return logmmse_stream_mode(fea_dim, device, lm, lm_block, lm_chan, li, lo);
        return logmmse_mode(fea_dim, device, lm, li, lo);
    }
    if (L < 2 || L > MAXLAYER - 1 || fea_dim < 1 || ctx < 1 || toff < 0 || toff >= ctx || cache < 1 || cache > MAXCACHEFRAME || bunch < 1) {
        printf("bpenhance: need layersizes (2..%d sizes), fea_dim, fea_context, 0 <= targ_offset < fea_context, traincache <= %d\n", MAXLAYER - 1, MAXCACHEFRAME);
        exit(0);
    }
    if (norm_file.empty() || wts_file.empty()) { printf("bpenhance: need norm_file and initwts_file\n"); exit(0); }
    if (list.empty() == (in_wav.empty() || out_wav.empty())) { printf("bpenhance: need wav_list, or in_wav and out_wav\n"); exit(0); }
    const int n_fft = 2 * (fea_dim - 1), hop = n_fft / 2;
    if (fea_dim < 33 || fea_dim > 1025 || (n_fft & (n_fft - 1))) { printf("bpenhance: 2*(fea_dim-1) must be a power of two from 64 to 2048\n"); exit(0); }
    if (ls[0] != ctx * fea_dim && ls[0] != (ctx + 1) * fea_dim) { printf("bpenhance: layersizes[0] must be fea_context*fea_dim (+ fea_dim with a NAT block)\n"); exit(0); }
    if (stream_chan > 1 && stream_block < 1) { printf("bpenhance: stream_chan needs stream_block\n"); exit(0); }
    if (stream_block > 0 && (long)stream_block * stream_chan > (1L << 28)) { printf("bpenhance: stream_block * stream_chan is too large\n"); exit(0); }
    if (forward == BP_FORWARD_ROWINV && compute == 1) { printf("bpenhance: forward=rowinv needs compute=fp32\n"); exit(0); }
    if (out_col < 0 || out_col + fea_dim > ls[L - 1]) { printf("bpenhance: out_col + fea_dim exceeds layersizes[last]\n"); exit(0); }

    // ---- inputs (all read and checked before the device is used)
    std::vector<std::string> ins, outs;
    read_wav_list(list, in_wav, out_wav, ins, outs);
    const int ns = (int)ins.size();
    std::vector<std::vector<float>> waves(ns);
    std::vector<int> rates(ns);
    for (int s = 0; s < ns; ++s) {
        const std::string err = bp::read_wav(ins[s], waves[s], rates[s]);
        if (!err.empty()) { printf("%s\n", err.c_str()); exit(0); }
        if (waves[s].empty()) { printf("%s: no samples\n", ins[s].c_str()); exit(0); }
        const size_t rows = (waves[s].size() - 1) / hop + 2 + ctx - 1;
        if (stream_block < 1 && rows > (size_t)cache) { printf("%s: %zu rows exceed traincache=%d (one sentence per call at most)\n", ins[s].c_str(), rows, cache); exit(0); }
    }
    std::vector<float> mean(fea_dim), istd(fea_dim);
    {
        // normalisation file: 1 header line, fea_dim means, 1 header line, fea_dim inverse std (as PfileReader reads it)
        FILE *fn = fopen(norm_file.c_str(), "rt");
        if (!fn) { printf("can not open normalization file: %s\n", norm_file.c_str()); exit(0); }
        char buff[256];
        bool ok = fgets(buff, sizeof(buff), fn) != nullptr;
        for (int j = 0; ok && j < fea_dim; ++j) { ok = fgets(buff, sizeof(buff), fn) != nullptr; mean[j] = (float)atof(buff); }
        ok = ok && fgets(buff, sizeof(buff), fn) != nullptr;
        for (int j = 0; ok && j < fea_dim; ++j) { ok = fgets(buff, sizeof(buff), fn) != nullptr; istd[j] = (float)atof(buff); }
        fclose(fn);
        if (!ok) { printf("normalization file too short\n"); exit(0); }
    }
    std::vector<std::vector<float>> Wv(L), Bv(L);
    float *weights[MAXLAYER] = {0}, *bias[MAXLAYER] = {0};
    for (int i = 1; i < L; ++i) { Wv[i].assign((size_t)ls[i] * ls[i - 1], 0.f); Bv[i].assign(ls[i], 0.f); weights[i] = Wv[i].data(); bias[i] = Bv[i].data(); }
    FILE *fi = fopen(wts_file.c_str(), "rb");
    if (!fi) { printf("can not open initial weights file: %s\n", wts_file.c_str()); exit(0); }
    const std::string err = bp::read_weights(fi, L, ls, weights, bias);
    fclose(fi);
    if (!err.empty()) { printf("%s\n", err.c_str()); exit(0); }

    bp_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.gpu_used = 1; cfg.numlayers = L;
    for (int i = 0; i < L; ++i) cfg.layersizes[i] = ls[i];
    cfg.bunchsize = bunch; cfg.lrate = 0.f; cfg.momentum = 0.f; cfg.dropoutflag = dropoutflag; cfg.visible_omit = vis; cfg.hid_omit = hid;
    cfg.activation = activation; cfg.device = device; cfg.compute_dtype = compute; cfg.max_chunk_frames = cache;
    bp_handle *h = nullptr;
    if (bp_create(&cfg, weights, bias, &h) != 0) { printf("%s\n", bp_last_error()); exit(0); }
    if (bp_set_output(h, out_act, out_lin, out_loss) != 0) { printf("%s\n", bp_last_error()); exit(0); }
    if (bp_set_forward(h, forward) != 0) { printf("%s\n", bp_last_error()); exit(0); }

    std::vector<float> pcm, out;
    std::vector<int> lens;
    size_t samples = 0;
    if (stream_block > 0) {
        // ---- a streaming session: channel c plays files c, c + stream_chan, ... one after the other
        bp_stream_config sc;
        memset(&sc, 0, sizeof(sc));
        sc.fea_dim = fea_dim; sc.context = ctx; sc.targ_offset = toff; sc.mean = mean.data(); sc.inv_std = istd.data();
        sc.target = target; sc.out_col = out_col; sc.n_chan = stream_chan; sc.max_push_samples = stream_block * stream_chan;
        bp_stream *st = nullptr;
        if (bp_stream_open(h, &sc, &st) != 0) { printf("%s\n", bp_last_error()); exit(0); }
        std::vector<std::vector<float>> enh;
        // a push returns what arrived plus, at the end of a sentence, the frames that waited for their look-ahead or the NAT row
        samples = play_files(st, bp_stream_push, stream_chan, stream_block, ins, waves, (size_t)stream_chan * ((size_t)stream_block + (size_t)(ctx + 8) * hop), enh);
        bp_stream_close(st);
        for (int s = 0; s < ns; ++s) {
            const std::string e = bp::write_wav(outs[s], enh[s].data(), waves[s].size(), rates[s]);
            if (!e.empty()) { printf("%s\n", e.c_str()); exit(0); }
        }
    }
    // ---- as many sentences per call as fit the chunk
    for (int s0 = stream_block > 0 ? ns : 0; s0 < ns;) {
        int s1 = s0;
        size_t rows = 0;
        pcm.clear(); lens.clear();
        while (s1 < ns) {
            const size_t r = (waves[s1].size() - 1) / hop + 2 + ctx - 1;
            if (rows + r > (size_t)cache) break;
            rows += r;
            pcm.insert(pcm.end(), waves[s1].begin(), waves[s1].end());
            lens.push_back((int)waves[s1].size());
            ++s1;
        }
        out.resize(pcm.size());
        bp_wave_chunk c;
        memset(&c, 0, sizeof(c));
        c.n_sent = s1 - s0; c.sent_len = lens.data(); c.pcm = pcm.data(); c.context = ctx; c.targ_offset = toff;
        c.mean = mean.data(); c.inv_std = istd.data(); c.target = target; c.out_col = out_col;
        if (bp_enhance_waves(h, fea_dim, &c, out.data(), nullptr) != 0) { printf("%s\n", bp_last_error()); exit(0); }
        size_t off = 0;
        for (int s = s0; s < s1; ++s) {
            const std::string e = bp::write_wav(outs[s], &out[off], waves[s].size(), rates[s]);
            if (!e.empty()) { printf("%s\n", e.c_str()); exit(0); }
            off += waves[s].size();
        }
        samples += pcm.size();
        s0 = s1;
    }
    bp_destroy(h);
    printf("bpenhance: %zu samples of %d sentences enhanced\n", samples, ns);
    return 1;
}
