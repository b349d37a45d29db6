// bpforward.cpp -- batch enhancement ("next" row N4 of SURVEY.md 8f): noisy log-power-spectrum Pfile in, enhanced
// log-power-spectrum Pfile out.  The reference keeps its decoder as an external download (README.md:39-44); the
// forward pass itself is cv_bunch_single (BP_GPU.cu:676-773: weights scaled by keep when the net was trained with
// dropout, linear output layer), which is what bp_forward_windows runs on the MI355X.  Input side = the reference's
// reader (Interface.cc:468-1034, via csrc/host/pfile_reader.cpp): mean/variance normalisation, fea_context stacked
// frames, optional noise-aware block; the output frame of a window is the one at offset targ_offset inside it.
//
//   bpforward fea_file=noisy.pfile norm_file=x.norm initwts_file=mlp.N.wts out_file=enh.pfile layersizes=1548,2048,...,129
//             fea_dim=129 fea_context=11 targ_offset=5 sent_range=0-99 [dropoutflag=1 visible_omit=0.1 hid_omit=0.2]
//             [bunchsize=1024] [traincache=102400] [activation=relu|sigmoid] [device=0] [compute=fp32|bf16]
//             [output_act=linear|sigmoid output_linear_dims=<n> output_loss=xent|mse]   (as the net was trained, bptrain.cpp)
//
// out_file: an ICSI Pfile with the input's sentence structure; sentence s holds one record per window of that
// sentence (frame id = window start + targ_offset), layersizes[last] features each: EVERY window of every sentence,
// exactly once, in file order (chunks are cut on sentence boundaries, PfileReader::plan_inference -- the training
// planner's cuts drop ctx-1 windows each, Interface.cc:607-614, which an enhancement tool must not).  Sentences shorter
// than the context contribute no records (as in the reader).  Errors: message + exit(0), success: return 1 (reference convention).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../../include/BP_GPU.h"
#include "keys.h"
#include "net_setup.h"
#include "pfile_reader.h"
#include "pfile_writer.h"
#include "wts_io.h"

int main(int argc, char **argv)
{
    std::string fea_file, norm_file, wts_file, out_file, range = "";
    int fea_dim = 0, ctx = 1, toff = 0, dropoutflag = 0, bunch = 1024, cache = 102400, L = 0, ls[MAXLAYER] = {0};
    int activation = 0, device = 0, compute = 0, out_act = 0, out_lin = 0, out_loss = 0;
    float vis = 0.f, hid = 0.f;
    using namespace bp;
    const Key keys[] = {
        {"fea_file", K_STR, &fea_file}, {"norm_file", K_STR, &norm_file}, {"initwts_file", K_STR, &wts_file},
        {"out_file", K_STR, &out_file}, {"sent_range", K_STR, &range},
        {"fea_dim", K_ATOI, &fea_dim}, {"fea_context", K_ATOI, &ctx}, {"targ_offset", K_ATOI, &toff}, {"dropoutflag", K_ATOI, &dropoutflag},
        {"visible_omit", K_ATOF, &vis}, {"hid_omit", K_ATOF, &hid},
        {"bunchsize", K_ATOI, &bunch}, {"traincache", K_ATOI, &cache},
        {"activation", K_IS, &activation, 0, 0, "sigmoid"}, {"device", K_ATOI, &device},
        {"compute", K_IS, &compute, 0, 0, "bf16"},
        {"layersizes", K_ATOI_SIZES, ls, 0, MAXLAYER, nullptr, nullptr, &L},
    };
    for (int i = 1; i < argc; ++i) {
        const Arg a = split_arg(argv[i]);
        // output layer (.wts files do not record it): the keys and checks of bptrain; other unknown names are ignored
        if (!key_apply(keys, "bpforward", a)) output_key(a, &out_act, &out_lin, &out_loss);
    }
    if (L < 2 || L > MAXLAYER - 1 || fea_dim < 1 || ctx < 1 || toff < 0 || toff >= ctx || cache < 1 || cache > MAXCACHEFRAME || bunch < 1) {
        printf("bpforward: need layersizes (2..%d sizes), fea_dim, fea_context, 0 <= targ_offset < fea_context, traincache <= %d\n", MAXLAYER - 1, MAXCACHEFRAME);
        exit(0);
    }
    const int sL = ls[L - 1];
    bp::ReaderConfig rc;
    rc.fea_file = fea_file; rc.targ_file = fea_file;          // no targets at enhancement time: the feature file stands in (unused)
    rc.norm_file = norm_file; rc.fea_dim = fea_dim; rc.fea_context = ctx; rc.targ_offset = toff; rc.out_dim = fea_dim;
    rc.traincache = cache; rc.input_dim = ls[0];
    bp::PfileReader reader(rc);
    reader.open();
    Weights wts(L, ls);
    const std::string err = load_weights(wts_file, L, ls, wts);
    if (!err.empty()) fail(err);
    int st = 0, en = (int)reader.total_sents() - 1;
    if (!range.empty()) { const size_t d = range.find('-'); if (d == std::string::npos) { printf("sent range: %s format error.\n", range.c_str()); exit(0); }
                          st = atoi(range.substr(0, d).c_str()); en = atoi(range.substr(d + 1).c_str()); }
    if (st < 0 || en >= (int)reader.total_sents() || st > en) { printf("sent range: %d to %d number error.\n", st, en); exit(0); }

    bp_config cfg = net_config(L, ls, bunch, cache, device);
    cfg.dropoutflag = dropoutflag; cfg.visible_omit = vis; cfg.hid_omit = hid; cfg.activation = activation; cfg.compute_dtype = compute;
    bp_handle *h = create_net(cfg, wts, out_act, out_lin, out_loss);

    // ---- output Pfile: records in reader order
    const std::vector<int> &fbs = reader.frames_before_sent();         // end offset (frames) of every sentence
    const int nsent = en - st + 1;
    bp::PfileWriter pw;
    if (!pw.open(out_file, nsent, sL)) fail("can not open output file: " + out_file);
    const bp::PfileReader::Plan plan = reader.plan_inference(st, en);    // every window exactly once (no training-style cut losses)
    bp::PfileReader::WindowChunk w;
    std::vector<float> out;
    unsigned total = 0;
    for (int c = 0; c < (int)plan.chunk_frame_st.size(); ++c) {
        const int n = reader.read_chunk_windows(plan, c, false, w);
        if (n <= 0) continue;
        bp_window_chunk d;
        memset(&d, 0, sizeof(d));
        d.n_samples = w.n_samples; d.n_frames = w.n_frames; d.fea_dim = w.fea_dim; d.context = ctx; d.n_nat = w.n_nat();
        d.fea = w.fea.data(); d.nat = w.nat.empty() ? nullptr : w.nat.data(); d.win_start = w.win_start.data();
        d.nat_row = w.nat_row.empty() ? nullptr : w.nat_row.data();
        out.resize((size_t)n * sL);
        check(bp_forward_windows(h, &d, out.data()));
        for (int i = 0; i < n; ++i) {
            const int gframe = plan.chunk_frame_st[c] + w.win_start[i];            // first frame of the window, file-global
            const int s = (int)(std::upper_bound(fbs.begin(), fbs.end(), gframe) - fbs.begin());
            const int s_begin = s == 0 ? 0 : fbs[s - 1];
            pw.add(s - st, gframe - s_begin + toff, &out[(size_t)i * sL]);
            ++total;
        }
    }
    pw.close();
    bp_destroy(h);
    printf("bpforward: %u frames of %d sentences enhanced -> %s\n", total, nsent, out_file.c_str());
    return 1;
}
