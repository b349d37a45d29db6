// bpfeat.cpp -- training features from audio: one WAV per line of wav_list -> one sentence of log-power-spectrum frames per
// WAV, in list order, in the Pfile format bptrain reads.  The analysis is bp_wave_lps, the same that bp_enhance_waves runs at
// enhancement time (include/bp_c_api.h), so training and enhancement see the same features.
//
//   bpfeat wav_list=noisy.list out_file=noisy.pfile fea_dim=129 [norm_out=noisy.norm] [device=0] [rate=8000]
//
// rate=R: every WAV whose sample rate is not R is converted to R on the device as the list is loaded
// (bp_resample_waves, one call and one line on stdout per distinct rate), and the features are those of the converted samples.
// Without the key a file's rate is not looked at.
// norm_out: per-bin mean and inverse standard deviation over all frames of the list (accumulated in double), in the
// normalisation-file format the reader takes as norm_file.  Errors: message + exit(0), success: return 1 (reference convention).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../../include/bp_c_api.h"
#include "corpus.h"
#include "keys.h"
#include "net_setup.h"
#include "pfile_writer.h"

int main(int argc, char **argv)
{
    std::string list, out_file, norm_out;
    int fea_dim = 0, device = 0, rate = 0;
    using namespace bp;
    const Key keys[] = {
        {"wav_list", K_STR, &list}, {"out_file", K_STR, &out_file}, {"norm_out", K_STR, &norm_out},
        {"fea_dim", K_ATOI, &fea_dim}, {"device", K_ATOI, &device},
        {"rate", K_INT, &rate, 1, (double)RATE_MAX, nullptr, RATE_TAIL},
    };
    for (int i = 1; i < argc; ++i) {
        const Arg a = split_arg(argv[i]);
        if (!key_apply(keys, "bpfeat", a)) fail("bpfeat: unknown key " + a.k);
    }
    if (list.empty() || out_file.empty() || !fea_dim_ok(fea_dim))
        fail("bpfeat: need wav_list, out_file and fea_dim (2*(fea_dim-1) a power of two from 64 to 2048)");
    // every WAV is read and checked before the device is used
    const std::vector<std::vector<float>> waves = read_wav_list("bpfeat", "wav list", list, nullptr, nullptr, rate, device);

    const int hop = fea_dim - 1, D = fea_dim, ns = (int)waves.size();
    bp::PfileWriter pw;
    if (!pw.open(out_file, ns, D)) fail("can not open output file: " + out_file);
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
        check(bp_wave_lps(device, D, s1 - s0, lens.data(), pcm.data(), lps.data()));
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
        if (!fn) fail("can not open norm file: " + norm_out);
        write_norm(fn, sum, sq, frames);
    }
    printf("bpfeat: %zu frames of %d sentences -> %s\n", frames, ns, out_file.c_str());
    return 1;
}
