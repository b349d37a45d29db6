// bppretrain.cpp -- layer-wise pre-training of a sigmoid net: the hidden layers of layersizes= become a stack
// of restricted Boltzmann machines (the first Gaussian-Bernoulli, the rest Bernoulli-Bernoulli), each trained with one-step
// contrastive divergence on the training sentences (the bp_rbm_* block of include/bp_c_api.h), and the result is written as a
// weights file that `bptrain initwts_file=` reads: the slot the reference's Perl driver fills with
// pretraining_weights/random_*.wts, which its toolbox can only make at random (toolbox/weights/gen_rand_net).
//
// bptrain's keys for the net and the feature side (numlayers layersizes bunchsize fea_dim fea_context targ_offset traincache
// init_randem_seed norm_file fea_file train_sent_range initwts_file outwts_file log_file; init_randem_*_min/max when there is no
// initwts_file; device, seed = the Philox key of the samples), read as bptrain reads them; no target file.  Its own keys are
// strict: rbm_epochs= rbm_lrate= rbm_momentum= rbm_weightcost= rbm_sample=, comma lists of one value or one per hidden layer; a
// value that does not parse or lies outside its range and an unknown rbm_ key end the run before the device is touched.
// For hidden layer 1 .. L-2 in turn: rbm_epochs passes over the chunks of train_sent_range in bptrain's shuffled order, one log
// line per pass with the mean reconstruction error per frame.  The output layer is initwts_file's (or the random one), unchanged.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "keys.h"
#include "net_setup.h"
#include "pfile_reader.h"
#include "wts_io.h"

using namespace bp;

static const char *TOOL = "bppretrain";

// one value or one per hidden layer -> one per hidden layer (index 1 .. n)
template <class T>
static std::vector<T> per_layer(const char *key, const std::vector<T> &given, int n, T dflt_first, T dflt_rest)
{
    std::vector<T> out(n + 1, dflt_rest);
    if (n >= 1) out[1] = dflt_first;
    if (given.empty()) return out;
    if ((int)given.size() != 1 && (int)given.size() != n)
        fail(std::string(TOOL) + ": " + key + " takes one value or one per hidden layer (" + std::to_string(n) + ")");
    for (int l = 1; l <= n; ++l) out[l] = given.size() == 1 ? given[0] : given[l - 1];
    return out;
}

int main(int argc, char **argv)
{
    std::string fea_file, norm_file, outwts_file, log_file, initwts_file, train_range;
    int fea_dim = 0, fea_context = 0, targ_offset = 0, traincache = 0, bunchsize = 0, seed = 0, device = 0, numlayers = 0;
    int layersizes[BP_MAXLAYER] = {0};
    float wmin = -0.1f, wmax = 0.1f, bmin = -0.1f, bmax = 0.1f;
    unsigned long long rbm_seed = 0;
    int epochs_v[BP_MAXLAYER], sample_v[BP_MAXLAYER], n_epochs = 0, n_sample = 0;
    std::vector<float> lrate_v, momentum_v, weightcost_v;
    const Key keys[] = {
        {"fea_file", K_STR, &fea_file}, {"norm_file", K_STR, &norm_file}, {"outwts_file", K_STR, &outwts_file},
        {"log_file", K_STR, &log_file}, {"initwts_file", K_STR, &initwts_file}, {"train_sent_range", K_STR, &train_range},
        {"fea_dim", K_ATOI, &fea_dim}, {"fea_context", K_ATOI, &fea_context}, {"targ_offset", K_ATOI, &targ_offset},
        {"traincache", K_ATOI, &traincache}, {"bunchsize", K_ATOI, &bunchsize}, {"init_randem_seed", K_ATOI, &seed},
        {"init_randem_weight_min", K_ATOF, &wmin}, {"init_randem_weight_max", K_ATOF, &wmax},
        {"init_randem_bias_min", K_ATOF, &bmin}, {"init_randem_bias_max", K_ATOF, &bmax},
        {"layersizes", K_ATOI_SIZES, layersizes, 0, BP_MAXLAYER, nullptr, nullptr, &numlayers},
        {"device", K_ATOI, &device}, {"seed", K_STRTOULL, &rbm_seed},
        {"rbm_lrate", K_FLOATS, &lrate_v}, {"rbm_momentum", K_FLOATS, &momentum_v}, {"rbm_weightcost", K_FLOATS, &weightcost_v},
    };
    for (int i = 1; i < argc; ++i) {
        const Arg a = split_arg(argv[i]);
        if (a.k == "layersizes") numlayers = 0;
        if (a.k == "rbm_epochs" || a.k == "rbm_sample") {
            const bool ep = a.k == "rbm_epochs";
            if (!parse_ints(a.v, 0, ep ? 100000 : 1, BP_MAXLAYER, ep ? epochs_v : sample_v, ep ? &n_epochs : &n_sample)) bad_value(TOOL, a.k, a.v);
            continue;
        }
        // unknown names are ignored, as bptrain ignores them (the Perl driver passes targ_file=, lrate=, ...), but not a
        // misspelt key of this tool's own
        if (!key_apply(keys, TOOL, a) && a.k.compare(0, 4, "rbm_") == 0) fail(std::string(TOOL) + ": unknown key " + a.k);
    }
    const int L = numlayers, NH = L - 2;                               // NH hidden layers = NH RBMs
    if (L < 3 || L > BP_MAXLAYER - 1) fail(std::string(TOOL) + ": layersizes: need 3.." + std::to_string(BP_MAXLAYER - 1) + " layer sizes");
    for (int l = 0; l < L; ++l)
        if (layersizes[l] < 1) fail(std::string(TOOL) + ": layersizes: a size is < 1");
    if (bunchsize < 1) fail(std::string(TOOL) + ": bunchsize must be >= 1");
    if (traincache < bunchsize || traincache > BP_MAXCACHEFRAME)
        fail(std::string(TOOL) + ": traincache must be in bunchsize.." + std::to_string(BP_MAXCACHEFRAME));
    if (device < 0) fail(std::string(TOOL) + ": device must be >= 0");
    bp_rbm_hyper d1, d2;
    check(bp_rbm_defaults(1, &d1));
    check(bp_rbm_defaults(2, &d2));
    const std::vector<int> epochs = per_layer<int>("rbm_epochs", std::vector<int>(epochs_v, epochs_v + n_epochs), NH, 10, 10);
    const std::vector<int> sample = per_layer<int>("rbm_sample", std::vector<int>(sample_v, sample_v + n_sample), NH, d1.sample, d2.sample);
    const std::vector<float> lrate = per_layer<float>("rbm_lrate", lrate_v, NH, d1.lrate, d2.lrate);
    const std::vector<float> momentum = per_layer<float>("rbm_momentum", momentum_v, NH, d1.momentum, d2.momentum);
    const std::vector<float> weightcost = per_layer<float>("rbm_weightcost", weightcost_v, NH, d1.weightcost, d2.weightcost);
    for (int l = 1; l <= NH; ++l) {
        if (lrate[l] < 0.0f) fail(std::string(TOOL) + ": rbm_lrate must be >= 0");
        if (weightcost[l] < 0.0f) fail(std::string(TOOL) + ": rbm_weightcost must be >= 0");
        if (!(momentum[l] >= 0.0f && momentum[l] < 1.0f)) fail(std::string(TOOL) + ": rbm_momentum must lie in [0, 1)");
    }

    FILE *log = fopen(log_file.c_str(), "wt");
    if (!log) fail("can not open output log file: " + log_file);
    FILE *fp_out = fopen(outwts_file.c_str(), "wb");
    if (!fp_out) { fprintf(log, "can not open output weights file: %s\n", outwts_file.c_str()); exit(0); }
    fprintf(log, "bppretrain: layersizes ");
    for (int j = 0; j < L; ++j) fprintf(log, "%d,", layersizes[j]);
    fprintf(log, " bunchsize %d traincache %d\n", bunchsize, traincache);
    for (int l = 1; l <= NH; ++l)
        fprintf(log, "RBM layer %d: %s visibles, epochs %d lrate %g momentum %g weightcost %g sample %d\n", l, l == 1 ? "Gaussian" : "Bernoulli",
                epochs[l], lrate[l], momentum[l], weightcost[l], sample[l]);

    // The reader pairs every feature frame with a target frame; there are no targets here, so the feature file stands in for
    // them (its frames are read as fea_dim-wide targets and dropped).
    ReaderConfig rc;
    rc.fea_file = fea_file; rc.targ_file = fea_file; rc.norm_file = norm_file;
    rc.fea_dim = fea_dim; rc.fea_context = fea_context; rc.targ_offset = targ_offset;
    rc.out_dim = fea_dim; rc.traincache = traincache; rc.input_dim = layersizes[0];
    PfileReader reader(rc);
    reader.open();

    Weights wts(L, layersizes);
    srand48(seed);                                      // once, for the random net and every shuffle, as in bptrain
    if (initwts_file.empty()) {
        random_weights(L, layersizes, wts.weights, wts.bias, wmin, wmax, bmin, bmax);
    } else {
        const std::string err = load_weights(initwts_file, L, layersizes, wts, log);
        if (!err.empty()) { fprintf(log, "%s\n", err.c_str()); exit(0); }
        fprintf(log, "Init weight file loaded.\n");
    }
    const size_t p = train_range.find('-');
    if (p == std::string::npos) { fprintf(log, "sent range: %s format error.\n", train_range.c_str()); exit(0); }
    const int st = atoi(train_range.substr(0, p).c_str()), en = atoi(train_range.substr(p + 1).c_str());
    const PfileReader::Plan tp = reader.plan(st, en);
    const int nchunks = (int)tp.chunk_frame_st.size();
    fprintf(log, "Get chunk info over: Training sentences have %d chunks, %d samples.\n", nchunks, (int)tp.total_samples);
    fflush(log);
    std::vector<int> chunk_index(nchunks);
    for (int i = 0; i < nchunks; ++i) chunk_index[i] = i;

    // ---- the device from here on
    bp_rbm_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.device = device; cfg.numlayers = L - 1;
    for (int l = 0; l < L - 1; ++l) cfg.layersizes[l] = layersizes[l];
    cfg.bunchsize = bunchsize; cfg.max_chunk_frames = traincache; cfg.seed = rbm_seed;
    bp_rbm *stack = nullptr;
    check(bp_rbm_create(&cfg, wts.weights, wts.bias, nullptr, &stack));
    std::vector<float> indata((size_t)layersizes[0] * traincache), dropped((size_t)fea_dim * traincache);
    PfileReader::WindowChunk w;
    for (int l = 1; l <= NH; ++l) {
        bp_rbm_hyper hy = {lrate[l], momentum[l], weightcost[l], l == 1 ? 0 : 1, sample[l]};
        check(bp_rbm_set_hyper(stack, l, &hy));
        for (int ep = 1; ep <= epochs[l]; ++ep) {
            PfileReader::rand_index(chunk_index.data(), nchunks);
            double err = 0.0;
            long frames = 0;
            for (int i = 0; i < nchunks; ++i) {
                const int n = reader.read_chunk_windows(tp, chunk_index[i], true, w);
                reader.expand(w, indata.data(), dropped.data());
                double e = 0.0;
                check(bp_rbm_train_chunk(stack, l, n, indata.data(), &e));
                err += e;
                frames += (long)(n / bunchsize) * bunchsize;
            }
            fprintf(log, "RBM layer %d epoch %d: reconstruction error per frame %.6f (%ld frames)\n", l, ep, frames ? err / frames : 0.0, frames);
            fflush(log);
        }
    }
    check(bp_rbm_get(stack, wts.weights, wts.bias, nullptr));        // (hidden layers 1 .. L-2; entry L-1 of the stack's arrays is not its own)
    bp_rbm_destroy(stack);
    fprintf(log, "Saving weights to file...\n");
    write_weights(fp_out, L, layersizes, wts.weights, wts.bias);
    fclose(fp_out);
    fprintf(log, "Saving over.\n");
    fclose(log);
    printf("all finish!\n");
    return 0;
}
