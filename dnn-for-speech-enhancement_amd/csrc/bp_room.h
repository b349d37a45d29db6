// bp_room.h -- what bp_room.hip shares with the mixing corpus (bp_set_mix_reverb, bp_mix.hip): the
// job record and the arguments of bp_mix_reverb_fir, the checks of a call's impulse responses, the job list and the launcher, for a
// unit that wants sentences it already holds on the device convolved.  Internal: nothing in here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

// one derived (reverberant) entry, or one sentence of bp_reverb_waves: n outputs at dst from the n source samples at src and the
// Lh taps at rir (delay d, early sum up to tap je); blk0: its first workgroup of bp_mix_reverb_fir
struct ReverbJob { int64_t src, dst, rir; int n, Lh, d, je, blk0, pad; };
struct ReverbArgs { const ReverbJob *job; int n_job; const float *src, *rir; float *out_r, *out_e; };

constexpr int RV_MAX_LEN = 1 << 30;                              // (sample indices of a sentence are ints on the device)

// the responses of a call, checked; off[k]: first tap of response k in rir_pcm, delay[k]
int check_rirs(const char *who, int n_rir, const int *rir_len, const float *rir_pcm, int early_taps, std::vector<int64_t> &off,
               std::vector<int> &delay);
// job k: n outputs at dst[k] from the sentence at src[k] and response rir[k]; returns the workgroups of the launch
int64_t fill_jobs(std::vector<ReverbJob> &job, const std::vector<int64_t> &off, const std::vector<int> &delay, const int *rir_len,
                  int early_taps);
hipError_t reverb_launch(const ReverbArgs &a, int64_t blocks, bool early, hipStream_t st);
