// bp_classic.h -- the log-MMSE recursion of bp_classic.hip, for bp_logmmse_waves (bp_classic.hip) and bp_eval_mix_logmmse
// (bp_mix.hip).  Definition: include/bp_c_api.h, INTEGRATION.md 1h.  Internal: nothing in here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "bp_handle.h"

// Checked parameters in the units the kernel uses (xi_min = 10^(xi_min_db / 10)).
struct LogmmseP { double alpha, mu, eta, xi_min, gamma_max; int init_frames; };
// The range rules of bp_logmmse_params (BP_ERR_ARG, nothing touched); p == null: the defaults.
int logmmse_check(const char *who, const bp_logmmse_params *p, LogmmseP &out);
// The recursion over the frames of n_sent sentences (frame prefix F [n_sent + 1], device) of the spectrum Y [frames][D]:
// gain [frames][D] = fl32(G), vad [frames] = fl32(vad_t).  One workgroup per sentence.
hipError_t logmmse_gain_launch(const LogmmseP &p, const float2 *Y, const int *F, int n_sent, int D, float *gain, float *vad, hipStream_t st);
