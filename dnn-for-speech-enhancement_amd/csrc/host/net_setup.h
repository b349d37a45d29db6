// What the net tools do between their arguments and the device: the host copy of the weights, the initial
// weights file, the normalisation file both ways, and the bp_config every tool starts from.  Errors end the run through
// bp::fail (keys.h) except where the caller chooses the destination of the message (load_weights).
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../../include/bp_c_api.h"
#include "keys.h"
#include "wts_io.h"

namespace bp {

// weights[l] and bias[l] of layers 1..L-1, zeroed, in the float *[] form of bp_create and wts_io.h
struct Weights {
    float *weights[BP_MAXLAYER] = {0}, *bias[BP_MAXLAYER] = {0};
    Weights(int L, const int *ls) : W_(L), B_(L)
    {
        for (int i = 1; i < L; ++i) {
            W_[i].assign((size_t)ls[i] * ls[i - 1], 0.f); B_[i].assign(ls[i], 0.f);
            weights[i] = W_[i].data(); bias[i] = B_[i].data();
        }
    }
    Weights(const Weights &) = delete;
    Weights &operator=(const Weights &) = delete;

private:
    std::vector<std::vector<float>> W_, B_;
};

// initwts_file into w: "" or the message, which the caller prints where its messages go (bptrain and bpmix: the log).
// progress: where `Loading Init weight file...` goes once the file is open (the training tools' log again), or null.
inline std::string load_weights(const std::string &path, int L, const int *ls, Weights &w, FILE *progress = nullptr)
{
    FILE *fi = fopen(path.c_str(), "rb");
    if (!fi) return "can not open initial weights file: " + path;
    if (progress) fprintf(progress, "Loading Init weight file...\n");
    const std::string err = read_weights(fi, L, ls, w.weights, w.bias);
    fclose(fi);
    return err;
}

// normalisation file: 1 header line, D means, 1 header line, D inverse std (as PfileReader reads it)
inline void read_norm(const std::string &path, int D, std::vector<float> &mean, std::vector<float> &istd)
{
    FILE *fn = fopen(path.c_str(), "rt");
    if (!fn) fail("can not open normalization file: " + path);
    char buff[1024];
    mean.assign(D, 0.f); istd.assign(D, 0.f);
    bool ok = fgets(buff, sizeof(buff), fn) != nullptr;
    for (int j = 0; ok && j < D; ++j) { ok = fgets(buff, sizeof(buff), fn) != nullptr; mean[j] = (float)atof(buff); }
    ok = ok && fgets(buff, sizeof(buff), fn) != nullptr;
    for (int j = 0; ok && j < D; ++j) { ok = fgets(buff, sizeof(buff), fn) != nullptr; istd[j] = (float)atof(buff); }
    fclose(fn);
    if (!ok) fail("normalization file too short");
}

// ... and written from the per-bin sums and sums of squares over n frames; closes fn
inline void write_norm(FILE *fn, const std::vector<double> &sum, const std::vector<double> &sq, size_t n)
{
    fprintf(fn, "<mean>\n");
    for (size_t j = 0; j < sum.size(); ++j) fprintf(fn, "%.9g\n", sum[j] / n);
    fprintf(fn, "<inverse std>\n");
    for (size_t j = 0; j < sum.size(); ++j) {
        const double m = sum[j] / n, var = sq[j] / n - m * m;
        fprintf(fn, "%.9g\n", var > 0.0 ? 1.0 / sqrt(var) : 1.0);
    }
    fclose(fn);
}

// one GPU, the net's shape and its sizes on the device; everything else zero, for the caller to set
inline bp_config net_config(int L, const int *ls, int bunchsize, int traincache, int device)
{
    bp_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.gpu_used = 1; cfg.numlayers = L;
    for (int i = 0; i < L; ++i) cfg.layersizes[i] = ls[i];
    cfg.bunchsize = bunchsize; cfg.max_chunk_frames = traincache; cfg.device = device;
    return cfg;
}

// the handle of a single-device tool: bp_create, then the output layer as the net was trained
inline bp_handle *create_net(const bp_config &cfg, Weights &w, int output_act, int output_linear_dims, int output_loss)
{
    bp_handle *h = nullptr;
    check(bp_create(&cfg, w.weights, w.bias, &h));
    check(bp_set_output(h, output_act, output_linear_dims, output_loss));
    return h;
}

// nat=dynamic (keys.h: nat_key) on the handle, with the tracker's defaults.  A net without the noise-aware block ends the run here,
// in the tool's name, and not at the first call that stages the block.  nat=static is the run without the key: nothing is called.
inline void set_nat(const char *tool, bp_handle *h, int nat, int context, int fea_dim, const int *ls)
{
    if (nat != BP_NAT_DYNAMIC) return;
    if ((long)ls[0] != (long)(context + 1) * fea_dim)
        fail(std::string(tool) + ": nat=dynamic needs a net with the noise-aware block: layersizes[0] = (fea_context+1)*fea_dim");
    check(bp_set_nat(h, BP_NAT_DYNAMIC, nullptr));
}

// post_gv / post_mask_* (keys.h: post_key, checked by check_post_keys) on the handle.  Without the keys nothing is called.
inline void set_post(bp_handle *h, const PostKeys &k, int fea_dim)
{
    if (!k.on()) return;
    bp_post_params p;
    check(bp_post_defaults(&p));
    std::vector<float> center, scale;
    if (!k.gv.empty()) {
        read_norm(k.gv, fea_dim, center, scale);
        p.gv = 1; p.gv_center = center.data(); p.gv_scale = scale.data();
    }
    p.mask_col = k.mask_col; p.mask_lo = k.lo; p.mask_hi = k.hi; p.mask_weight = k.weight;
    check(bp_set_post(h, fea_dim, &p));
}

// the GV factors in norm-file format (bpeval gv_out=; read back by read_norm as post_gv=): centre, then scale
inline void write_gv(const std::string &path, const std::vector<float> &center, const std::vector<float> &scale)
{
    FILE *fn = fopen(path.c_str(), "wt");
    if (!fn) fail("can not open GV file: " + path);
    fprintf(fn, "<gv center>\n");
    for (float v : center) fprintf(fn, "%.9g\n", v);
    fprintf(fn, "<gv scale>\n");
    for (float v : scale) fprintf(fn, "%.9g\n", v);
    fclose(fn);
}

}  // namespace bp
