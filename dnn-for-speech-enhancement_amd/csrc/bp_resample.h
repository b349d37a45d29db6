// bp_resample.h -- the rational sample-rate converter of bp_resample.hip (bp_resample_waves; include/bp_c_api.h): the
// kernel's arguments, the plan of a call and the launcher, for a unit that wants to convert what it already holds on the device.
// Internal: nothing in here is part of the C ABI.
//
// Device layout of one call: sentence s starts at float offset off[s] of the PCM block, 16-byte aligned, and is followed by
// zeros up to the next multiple of four samples, so that a workgroup fetches its span with 16-byte loads; its n_out[s] output
// samples lie at oo[s] of the output block, back to back, the layout the caller gets.  Workgroup b of the flat grid serves
// RS_BLOCK consecutive output samples of the sentence s with rb[s] <= b < rb[s + 1], one per lane.
//
// Taps in polyphase order: an output sample with phase r = (k q + Lh) mod p meets the taps r, r + p, r + 2p, ... and nothing
// else, so hp[r * tpp + i] = h[r + i p] (tpp = ceil(taps / p) entries per phase, the unused tail zero and never read) lets a lane
// walk consecutive floats.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/bp_c_api.h"

constexpr int RS_BLOCK = 256;              // output samples per workgroup, one per lane
constexpr int RS_LDS_FLOATS = 16000;       // the largest input span a workgroup stages in LDS (64 000 bytes); longer: from global

struct ResampleArgs {
    const float *pcm;                       // the sentences in the padded layout above
    const float *hp;                        // [p][tpp] polyphase taps
    const int64_t *off;                     // [n_sent] first sample of sentence s in pcm
    const int *len;                         // [n_sent] samples of sentence s
    const int *oo;                          // [n_sent + 1] first output sample of sentence s in out
    const int *rb;                          // [n_sent + 1] first workgroup of sentence s
    float *out;
    int n_sent, p, q, Lh, taps, tpp;
    int lds;                                // 1: every workgroup's span fits RS_LDS_FLOATS and is staged; 0: read from global
};

struct ResamplePlan {
    int p, q, Lh, taps, tpp, lds;
    std::vector<float> hp;                  // [p * tpp]
    std::vector<int64_t> off;               // [n_sent]
    std::vector<int> oo, rb;                // [n_sent + 1]
    size_t in_floats, lds_bytes;            // padded samples of the call; dynamic LDS of a workgroup (0 without staging)
};
// The plan of a call whose arguments bp_resample_waves has checked (ratio, parameters, lengths, the total below 2^31).
void resample_plan(int p, int q, const bp_resample_params &prm, int n_sent, const int *sent_len, ResamplePlan &rp);
hipError_t resample_launch(const ResampleArgs &a, const ResamplePlan &rp, hipStream_t st);
