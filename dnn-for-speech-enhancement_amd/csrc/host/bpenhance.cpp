// bpenhance.cpp -- waveform enhancement: noisy WAV in, enhanced WAV out, on the MI355X through bp_enhance_waves (analysis,
// the forward of bpforward, resynthesis, overlap-add; include/bp_c_api.h).
//
//   bpenhance norm_file=x.norm initwts_file=mlp.N.wts layersizes=1548,2048,2048,2048,129 fea_dim=129 fea_context=11
//             targ_offset=5 (wav_list=<"in.wav out.wav" per line> | in_wav=noisy.wav out_wav=enh.wav)
//             [wave_target=lps|mask] [out_col=0] [dropoutflag=1 visible_omit=0.1 hid_omit=0.2] [bunchsize=1024]
//             [traincache=102400] [activation=relu|sigmoid] [device=0] [compute=fp32|bf16]
//             [output_act=linear|sigmoid output_linear_dims=<n> output_loss=xent|mse]   (as the net was trained, bptrain.cpp)
//             [stream_block=<samples> [stream_chan=<n>]] [forward=default|rowinv] [rate=8000] [nat=static|dynamic]
//             [post_gv=gv.norm] [post_mask_col=129 [post_mask_lo=0.5] [post_mask_hi=0.5] [post_mask_weight=1]]
//   bpenhance method=logmmse fea_dim=129 (wav_list=... | in_wav=... out_wav=...) [device=0] [lm_alpha=0.98] [lm_mu=0.98]
//             [lm_eta=0.15] [lm_xi_min_db=-25] [lm_gamma_max=40] [lm_init_frames=6] [lm_stream_block=<samples> [lm_stream_chan=<n>]]
//             [lm_noise=vad|spp]
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
// files hold the bytes of a run without the key.  lm_noise=spp gives the baseline, streamed or not, the MMSE-SPP noise tracker
// (bp_logmmse_waves_nt, bp_lmstream_open_nt); vad, the default, is a run without the key.
// rate=R: the rate the net works at.  A file at another rate f is converted to R on the device
// (bp_resample_waves), enhanced, converted back to f, trimmed to its original length and written at f as without the key; what it
// held above R/2 is gone.  One call and one line on stdout per distinct rate and direction.  Not with stream_block or
// lm_stream_block (a stream needs a filter that keeps state), and not with method=logmmse.
// post_gv / post_mask_* (wave_target=lps): the net's LPS estimate is post-processed before resynthesis
// (bp_set_post) -- GV equalisation with the factors of the file that `bpeval gv_out=` wrote, and the mask gate on the columns from
// post_mask_col on; a streaming session opened below keeps them.  Without the keys the output is that of a run before they existed.
// Errors: message + exit(0), success: return 1 (reference convention).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../../include/BP_GPU.h"
#include "corpus.h"
#include "keys.h"
#include "net_setup.h"
#include "wav_io.h"

using namespace bp;
static const char *const WHO = "bpenhance";

// the input and output files of wav_list, or the one pair
static void wav_pairs(const std::string &list, const std::string &in_wav, const std::string &out_wav, std::vector<std::string> &ins,
                          std::vector<std::string> &outs)
{
    if (list.empty()) { ins.push_back(in_wav); outs.push_back(out_wav); return; }
    read_pairs(WHO, "wav list", "wav list", "an input and an output file", list, ins, outs);
}

// method=logmmse: every file through bp_logmmse_waves, as many sentences per call as stay below MAXCACHEFRAME frames
static int logmmse_mode(int fea_dim, int device, const bp_logmmse_params &lm, const bp_noise_params *nz, const std::vector<std::string> &ins, const std::vector<std::string> &outs)
{
    const int ns = (int)ins.size(), hop = fea_dim - 1;
    std::vector<std::vector<float>> waves(ns);
    std::vector<int> rates(ns);
    for (int s = 0; s < ns; ++s) {
        waves[s] = read_one(WHO, ins[s], &rates[s]);
        if (waves[s].size() > (size_t)1 << 30) fail(ins[s] + ": too long");
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
        if (nz) check(bp_logmmse_waves_nt(device, fea_dim, &lm, nz, s1 - s0, lens.data(), pcm.data(), out.data(), nullptr, nullptr, nullptr));
        else check(bp_logmmse_waves(device, fea_dim, &lm, s1 - s0, lens.data(), pcm.data(), out.data(), nullptr, nullptr));
        size_t off = 0;
        for (int s = s0; s < s1; ++s) {
            const std::string e = bp::write_wav(outs[s], &out[off], waves[s].size(), rates[s]);
            if (!e.empty()) fail(e);
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
        check(push(st, n_in.data(), pcm.data(), end.data(), n_out.data(), out.data(), out.size()));
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
static int logmmse_stream_mode(int fea_dim, int device, const bp_logmmse_params &lm, const bp_noise_params *nz, int block, int chan, const std::vector<std::string> &ins,
                               const std::vector<std::string> &outs)
{
    const int ns = (int)ins.size(), hop = fea_dim - 1;
    std::vector<std::vector<float>> waves(ns), enh;
    std::vector<int> rates(ns);
    for (int s = 0; s < ns; ++s) {
        waves[s] = read_one(WHO, ins[s], &rates[s]);
    }
    bp_lmstream *st = nullptr;
    if (nz) check(bp_lmstream_open_nt(device, fea_dim, &lm, nz, chan, block * chan, &st));
    else check(bp_lmstream_open(device, fea_dim, &lm, chan, block * chan, &st));
    // a push returns what arrived plus what waited for the noise start or for the end of the sentence
    const size_t samples = play_files(st, bp_lmstream_push, chan, block, ins, waves, (size_t)chan * ((size_t)block + ((size_t)lm.init_frames + 1) * hop), enh);
    bp_lmstream_close(st);
    for (int s = 0; s < ns; ++s) {
        const std::string e = bp::write_wav(outs[s], enh[s].data(), waves[s].size(), rates[s]);
        if (!e.empty()) fail(e);
    }
    printf("bpenhance: %zu samples of %d sentences enhanced (logmmse, streamed)\n", samples, ns);
    return 1;
}

int main(int argc, char **argv)
{
    std::string norm_file, wts_file, list, in_wav, out_wav;
    int logmmse = 0;
    std::vector<std::string> given;
    bp_logmmse_params lm;
    bp_logmmse_defaults(&lm);
    int fea_dim = 0, ctx = 1, toff = 0, dropoutflag = 0, bunch = 1024, cache = 102400, L = 0, ls[MAXLAYER] = {0};
    int activation = 0, device = 0, compute = 0, out_act = 0, out_lin = 0, out_loss = 0, target = BP_WAVE_LPS, out_col = 0;
    int stream_block = 0, stream_chan = 1, forward = BP_FORWARD_DEFAULT, lm_block = 0, lm_chan = 1, rate = 0;
    bool lm_chan_given = false;
    int lm_noise = BP_NOISE_VAD, nat = BP_NAT_STATIC;
    PostKeys post;
    float vis = 0.f, hid = 0.f;
    const char *const count = "is not a count >= 1";
    const Key keys[] = {
        {"method", K_CHOICE, &logmmse, 0, 0, "net|logmmse", "is not net or logmmse"},
        {"lm_stream_block", K_INT, &lm_block, 1, 1 << 24, nullptr, count}, {"lm_stream_chan", K_INT, &lm_chan, 1, 1 << 24, nullptr, count},
        {"norm_file", K_STR, &norm_file}, {"initwts_file", K_STR, &wts_file},
        {"wav_list", K_STR, &list}, {"in_wav", K_STR, &in_wav}, {"out_wav", K_STR, &out_wav},
        {"fea_dim", K_ATOI, &fea_dim}, {"fea_context", K_ATOI, &ctx}, {"targ_offset", K_ATOI, &toff}, {"dropoutflag", K_ATOI, &dropoutflag},
        {"visible_omit", K_ATOF, &vis}, {"hid_omit", K_ATOF, &hid},
        {"bunchsize", K_ATOI, &bunch}, {"traincache", K_ATOI, &cache},
        {"activation", K_IS, &activation, 0, 0, "sigmoid"}, {"device", K_ATOI, &device},
        {"compute", K_IS, &compute, 0, 0, "bf16"},
        {"out_col", K_ATOI, &out_col},
        {"stream_block", K_INT, &stream_block, 1, 1 << 24, nullptr, count}, {"stream_chan", K_INT, &stream_chan, 1, 1 << 24, nullptr, count},
        {"forward", K_CHOICE, &forward, BP_FORWARD_DEFAULT, 0, "default|rowinv", "is not default or rowinv"},
        {"wave_target", K_CHOICE, &target, BP_WAVE_LPS, 0, "lps|mask", "is not lps or mask"},
        {"layersizes", K_ATOI_SIZES, ls, 0, MAXLAYER, nullptr, nullptr, &L},
        {"rate", K_INT, &rate, 1, (double)RATE_MAX, nullptr, RATE_TAIL},
    };
    for (int i = 1; i < argc; ++i) {
        const Arg a = split_arg(argv[i]);
        const std::string &k = a.k, &v = a.v;
        given.push_back(k);
        if (k == "lm_stream_chan") lm_chan_given = true;
        // output layer (.wts files do not record it): the keys and checks of bptrain
        if (key_apply(keys, WHO, a) || output_key(a, &out_act, &out_lin, &out_loss) || lm_noise_key(a, WHO, "is not vad or spp", &lm_noise) ||
            nat_key(a, WHO, "is not static or dynamic", &nat) || post_key(a, WHO, true, &post)) continue;
        // the log-MMSE parameters stay by hand: any lm_ name is a number first (nan and inf included), and only then a known key
        if (k.compare(0, 3, "lm_") != 0) fail("bpenhance: unknown key " + k);
        char *end = nullptr;
        const double d = strtod(v.c_str(), &end);
        if (v.empty() || *end) fail(k + ": " + v + " is not a number");
        if (k == "lm_alpha") lm.alpha = d; else if (k == "lm_mu") lm.mu = d; else if (k == "lm_eta") lm.eta = d;
        else if (k == "lm_xi_min_db") lm.xi_min_db = d; else if (k == "lm_gamma_max") lm.gamma_max = d;
        else if (k == "lm_init_frames") {
            if (!(d >= -1e9 && d <= 1e9) || d != (double)(int)d) fail(k + ": " + v + " is not a count");
            lm.init_frames = (int)d;
        }
        else fail("bpenhance: unknown key " + k);
    }
    if (rate && (stream_block > 0 || lm_block > 0))
        fail("bpenhance: rate does not go with stream_block or lm_stream_block (a stream needs a sample-rate converter that keeps state)");
    for (const std::string &k : given) {
        const bool lm_key = k.compare(0, 3, "lm_") == 0;
        if (!logmmse && lm_key) fail("bpenhance: " + k + " needs method=logmmse");
        if (logmmse && !lm_key && k != "method" && k != "fea_dim" && k != "device" && k != "wav_list" && k != "in_wav" && k != "out_wav") {
            fail("bpenhance: method=logmmse takes no " + k + " (only fea_dim, device, wav_list or in_wav and out_wav, and the lm_ keys, lm_stream_block and lm_stream_chan among them)");
        }
    }
    if (logmmse) {
        if (list.empty() == (in_wav.empty() || out_wav.empty())) fail("bpenhance: need wav_list, or in_wav and out_wav");
        if (!fea_dim_ok(fea_dim)) fail("bpenhance: 2*(fea_dim-1) must be a power of two from 64 to 2048");
        if (lm_chan_given && lm_block < 1) fail("bpenhance: lm_stream_chan needs lm_stream_block");
        if (lm_block > 0 && ((long)lm_block * lm_chan > (1L << 28) || lm_chan > (1 << 16))) fail("bpenhance: lm_stream_block * lm_stream_chan is too large");
        std::vector<std::string> li, lo;
        wav_pairs(list, in_wav, out_wav, li, lo);
        bp_noise_params nz;                                      // lm_noise=vad: the calls without noise parameters
        bp_noise_defaults(&nz);
        nz.mode = lm_noise;
        const bp_noise_params *np = lm_noise != BP_NOISE_VAD ? &nz : nullptr;
        if (lm_block > 0) return logmmse_stream_mode(fea_dim, device, lm, np, lm_block, lm_chan, li, lo);
        return logmmse_mode(fea_dim, device, lm, np, li, lo);
    }
    if (L < 2 || L > MAXLAYER - 1 || fea_dim < 1 || ctx < 1 || toff < 0 || toff >= ctx || cache < 1 || cache > MAXCACHEFRAME || bunch < 1) {
        printf("bpenhance: need layersizes (2..%d sizes), fea_dim, fea_context, 0 <= targ_offset < fea_context, traincache <= %d\n", MAXLAYER - 1, MAXCACHEFRAME);
        exit(0);
    }
    if (norm_file.empty() || wts_file.empty()) fail("bpenhance: need norm_file and initwts_file");
    if (list.empty() == (in_wav.empty() || out_wav.empty())) fail("bpenhance: need wav_list, or in_wav and out_wav");
    const int n_fft = 2 * (fea_dim - 1), hop = n_fft / 2;
    if (!fea_dim_ok(fea_dim)) fail("bpenhance: 2*(fea_dim-1) must be a power of two from 64 to 2048");
    if (ls[0] != ctx * fea_dim && ls[0] != (ctx + 1) * fea_dim) fail("bpenhance: layersizes[0] must be fea_context*fea_dim (+ fea_dim with a NAT block)");
    if (stream_chan > 1 && stream_block < 1) fail("bpenhance: stream_chan needs stream_block");
    if (stream_block > 0 && (long)stream_block * stream_chan > (1L << 28)) fail("bpenhance: stream_block * stream_chan is too large");
    if (forward == BP_FORWARD_ROWINV && compute == 1) fail("bpenhance: forward=rowinv needs compute=fp32");
    if (out_col < 0 || out_col + fea_dim > ls[L - 1]) fail("bpenhance: out_col + fea_dim exceeds layersizes[last]");
    check_post_keys(WHO, post, target);
    if (post.mask_col >= 0 && post.mask_col + fea_dim > ls[L - 1]) fail("bpenhance: post_mask_col + fea_dim exceeds layersizes[last]");

    // ---- inputs (all read and checked before the device is used)
    std::vector<std::string> ins, outs;
    wav_pairs(list, in_wav, out_wav, ins, outs);
    const int ns = (int)ins.size();
    std::vector<std::vector<float>> waves(ns);
    std::vector<int> rates(ns);
    for (int s = 0; s < ns; ++s) {
        waves[s] = read_one(WHO, ins[s], &rates[s]);
        size_t n_net = waves[s].size();                          // samples at the net's rate
        if (rate && rates[s] != rate) {
            check_convertible(WHO, ins[s], rates[s], rate);
            if (waves[s].size() > (size_t)INT32_MAX) fail(ins[s] + ": too long to convert");
            int p = 0, q = 0;
            int64_t no = 0;
            check(bp_resample_ratio(rates[s], rate, &p, &q));
            check(bp_resample_len((int64_t)waves[s].size(), p, q, &no));
            n_net = (size_t)no;
        }
        const size_t rows = (n_net - 1) / hop + 2 + ctx - 1;
        if (stream_block < 1 && rows > (size_t)cache) { printf("%s: %zu rows exceed traincache=%d (one sentence per call at most)\n", ins[s].c_str(), rows, cache); exit(0); }
    }
    std::vector<float> mean, istd;
    read_norm(norm_file, fea_dim, mean, istd);
    Weights wts(L, ls);
    const std::string err = load_weights(wts_file, L, ls, wts);
    if (!err.empty()) fail(err);

    bp_config cfg = net_config(L, ls, bunch, cache, device);
    cfg.dropoutflag = dropoutflag; cfg.visible_omit = vis; cfg.hid_omit = hid; cfg.activation = activation; cfg.compute_dtype = compute;
    bp_handle *h = create_net(cfg, wts, out_act, out_lin, out_loss);
    check(bp_set_forward(h, forward));
    set_nat(WHO, h, nat, ctx, fea_dim, ls);                      // (a stream opened below keeps the mode, as it keeps the forward's)
    set_post(h, post, fea_dim);                                  // (... and the post-processing)

    std::vector<float> pcm, out;
    std::vector<int> lens;
    size_t samples = 0;
    std::vector<size_t> orig_len(ns);                            // rate=: the files as they came, and what the net made of them
    std::vector<std::vector<float>> enh(rate ? ns : 0);
    for (int s = 0; s < ns; ++s) orig_len[s] = waves[s].size();
    if (rate) convert_rates(WHO, "input", device, rate, waves, rates);
    if (stream_block > 0) {
        // ---- a streaming session: channel c plays files c, c + stream_chan, ... one after the other
        bp_stream_config sc;
        memset(&sc, 0, sizeof(sc));
        sc.fea_dim = fea_dim; sc.context = ctx; sc.targ_offset = toff; sc.mean = mean.data(); sc.inv_std = istd.data();
        sc.target = target; sc.out_col = out_col; sc.n_chan = stream_chan; sc.max_push_samples = stream_block * stream_chan;
        bp_stream *st = nullptr;
        check(bp_stream_open(h, &sc, &st));
        std::vector<std::vector<float>> enh;
        // a push returns what arrived plus, at the end of a sentence, the frames that waited for their look-ahead or the NAT row
        samples = play_files(st, bp_stream_push, stream_chan, stream_block, ins, waves, (size_t)stream_chan * ((size_t)stream_block + (size_t)(ctx + 8) * hop), enh);
        bp_stream_close(st);
        for (int s = 0; s < ns; ++s) {
            const std::string e = bp::write_wav(outs[s], enh[s].data(), waves[s].size(), rates[s]);
            if (!e.empty()) fail(e);
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
        check(bp_enhance_waves(h, fea_dim, &c, out.data(), nullptr));
        size_t off = 0;
        for (int s = s0; s < s1; ++s) {
            if (rate) enh[s].assign(out.begin() + off, out.begin() + off + waves[s].size());
            else {
                const std::string e = bp::write_wav(outs[s], &out[off], waves[s].size(), rates[s]);
                if (!e.empty()) fail(e);
            }
            off += waves[s].size();
        }
        samples += pcm.size();
        s0 = s1;
    }
    if (rate) {                                                  // back to every file's own rate, trimmed to its own length
        convert_rates(WHO, "output", device, rate, enh, rates, rate);
        for (int s = 0; s < ns; ++s) {
            const std::string e = bp::write_wav(outs[s], enh[s].data(), orig_len[s], rates[s]);
            if (!e.empty()) fail(e);
        }
    }
    bp_destroy(h);
    printf("bpenhance: %zu samples of %d sentences enhanced\n", samples, ns);
    return 1;
}
