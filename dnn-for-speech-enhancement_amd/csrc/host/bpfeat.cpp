// bpfeat.cpp -- training features from audio: one WAV per line of wav_list -> one sentence of log-power-spectrum frames per
// WAV, in list order, in the Pfile format bptrain reads.  The analysis is bp_wave_lps, the same that bp_enhance_waves runs at
// enhancement time (include/bp_c_api.h), so training and enhancement see the same features.
//
//   bpfeat wav_list=noisy.list out_file=noisy.pfile fea_dim=129 [norm_out=noisy.norm] [device=0]
//
// norm_out: per-bin mean and inverse standard deviation over all frames of the list (accumulated in double), in the
// normalisation-file format the reader takes as norm_file.  Errors: message + exit(0), success: return 1 (reference convention).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../../include/bp_c_api.h"
#include "pfile_writer.h"
#include "wav_io.h"

int main(int argc, char **argv)
{
    std::string list, out_file, norm_out;
    int fea_dim = 0, device = 0;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { printf("Arg: %s  Format Error\n", argv[i]); exit(0); }
        const std::string k(argv[i], eq - argv[i]), v(eq + 1);
        if (k == "wav_list") list = v; else if (k == "out_file") out_file = v; else if (k == "norm_out") norm_out = v;
        else if (k == "fea_dim") fea_dim = atoi(v.c_str()); else if (k == "device") device = atoi(v.c_str());
        else { printf("bpfeat: unknown key %s\n", k.c_str()); exit(0); }
    }
    const int n_fft = 2 * (fea_dim - 1);
    if (list.empty() || out_file.empty() || fea_dim < 33 || fea_dim > 1025 || (n_fft & (n_fft - 1))) {
        printf("bpfeat: need wav_list, out_file and fea_dim (2*(fea_dim-1) a power of two from 64 to 2048)\n");
        exit(0);
    }
    // every WAV is read and checked before the device is used
    FILE *fl = fopen(list.c_str(), "rt");
    if (!fl) { printf("can not open wav list: %s\n", list.c_str()); exit(0); }
    std::vector<std::vector<float>> waves;
    char line[4096];
    while (fgets(line, sizeof(line), fl)) {
        std::string p(line);
        while (!p.empty() && (p.back() == '\n' || p.back() == '\r' || p.back() == ' ' || p.back() == '\t')) p.pop_back();
        if (p.empty()) continue;
        waves.emplace_back();
        int sr = 0;
        const std::string err = bp::read_wav(p, waves.back(), sr);
        if (!err.empty()) { printf("%s\n", err.c_str()); exit(0); }
        if (waves.back().empty()) { printf("%s: no samples\n", p.c_str()); exit(0); }
    }
    fclose(fl);
    if (waves.empty()) { printf("bpfeat: %s lists no wav file\n", list.c_str()); exit(0); }

    const int hop = n_fft / 2, D = fea_dim, ns = (int)waves.size();
    bp::PfileWriter pw;
    if (!pw.open(out_file, ns, D)) { printf("can not open output file: %s\n", out_file.c_str()); exit(0); }
    std::vector<double> sum(D, 0.0), sq(D, 0.0);
    size_t frames = 0;
    // sentences in batches of about 2^24 samples per call
    std::vector<float> pcm, lps;
    std::vector<int> lens;
    for (int s0 = 0; s0 < ns;) {
        int s1 = s0;
        size_t n = 0, T = 0;
        pcm.clear(); lens.clear();
        while (s1 < ns && (s1 == s0 || n + waves[s1].size() <= ((size_t)1 << 24))) {
            pcm.insert(pcm.end(), waves[s1].begin(), waves[s1].end());
            lens.push_back((int)waves[s1].size());
            n += waves[s1].size(); T += (waves[s1].size() - 1) / hop + 2;
            ++s1;
        }
        lps.resize(T * D);
        if (bp_wave_lps(device, D, s1 - s0, lens.data(), pcm.data(), lps.data()) != 0) { printf("%s\n", bp_last_error()); exit(0); }
        size_t f = 0;
        for (int s = s0; s < s1; ++s) {
            const int Ts = (int)((waves[s].size() - 1) / hop + 2);
            for (int t = 0; t < Ts; ++t, ++f) {
                const float *row = &lps[f * D];
                pw.add(s, t, row);
                for (int k = 0; k < D; ++k) { sum[k] += row[k]; sq[k] += (double)row[k] * row[k]; }
            }
        }
        frames += T;
        s0 = s1;
    }
    pw.close();
    if (!norm_out.empty()) {
        FILE *fn = fopen(norm_out.c_str(), "wt");
        if (!fn) { printf("can not open norm file: %s\n", norm_out.c_str()); exit(0); }
        fprintf(fn, "<mean>\n");
        for (int k = 0; k < D; ++k) fprintf(fn, "%.9g\n", sum[k] / frames);
        fprintf(fn, "<inverse std>\n");
        for (int k = 0; k < D; ++k) {
            const double m = sum[k] / frames, var = sq[k] / frames - m * m;
            fprintf(fn, "%.9g\n", var > 0.0 ? 1.0 / sqrt(var) : 1.0);
        }
        fclose(fn);
    }
    printf("bpfeat: %zu frames of %d sentences -> %s\n", frames, ns, out_file.c_str());
    return 1;
}
