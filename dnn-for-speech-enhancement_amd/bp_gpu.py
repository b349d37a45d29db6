"""Host-side mirror of the reference's `BP_GPU` class (BP_GPU.h:40-88) over the C ABI in
include/bp_c_api.h (ctypes binding of libbp_hip.so, the gfx950 HIP library).

Same constructor argument order, method names, argument meaning and error behaviour as the
reference object so callers/tests read like `BPtrain.cc`:

    obj = BP_GPU(gpu_used, numlayers, layersizes, bunchsize, lrate, momentum, weightcost,
                 weights, bias, dropoutflag, visible_omit, hid_omit)
    obj.train(n_frames, indata, targ)             # BP_GPU.cu:241-331
    err = obj.CrossValid(n_frames, indata, targ)  # BP_GPU.cu:408-479 (SUM of squared errors)
    obj.returnWeights(weights, bias)              # BP_GPU.cu:910-923

There is NO CPU fallback: if the HIP library is missing or no MI355X is visible the
constructor raises.  (The reference prints and calls exit(0) on errors, BP_GPU.cu:20-24;
`strict_exit=True` reproduces that, the default raises BPError so Python callers can react.)
"""
import ctypes as C
import os
import sys

import numpy as np

MAXLAYER = 10          # BP_GPU.h:13
MAXCACHEFRAME = 200000  # BP_GPU.h:14

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libbp_hip.so")

# every symbol include/bp_c_api.h declares
ABI_SYMBOLS = [
    "bp_last_error", "bp_abi_version", "bp_build_target", "bp_create", "bp_destroy", "bp_train_chunk",
    "bp_cv_chunk", "bp_forward", "bp_get_weights", "bp_get_deltas", "bp_upload_chunk",
    "bp_fill_chunk_synthetic", "bp_train_resident", "bp_sync", "bp_grads_resident",
    "bp_grad_layout", "bp_grad_floats", "bp_read_grads", "bp_read_layer_output", "bp_last_train_ms", "bp_time_kernel",
    "bp_upload_chunk_windows", "bp_train_chunk_windows", "bp_cv_chunk_windows",
    "bp_set_hyper", "bp_set_output", "bp_set_forward", "bp_dp_attach", "bp_dp_attach_ex", "bp_dp_detach", "bp_dp_info", "bp_dp_peer_info", "bp_dp_handoff", "bp_dp_barrier", "bp_dp_allgather",
    "bp_rdv_open", "bp_rdv_barrier", "bp_rdv_allgather", "bp_rdv_close", "bp_device_pci_bus_id", "bp_host_register", "bp_host_unregister",
    "bp_profile_step", "bp_measure_peaks", "bp_device_count", "bp_train_resident_masked", "bp_forward_windows",
    "bp_enhance_waves", "bp_wave_lps",
    "bp_set_mix_corpus", "bp_train_mix", "bp_cv_mix", "bp_mix_features", "bp_mix_plan", "bp_mix_shuffle",
    "bp_set_mix_reverb", "bp_reverb_waves", "bp_mix_rir_delay", "bp_mix_reverb_pairs",
    "bp_rir_image", "bp_rir_orders", "bp_rir_beta", "bp_rir_rooms",
    "bp_score_waves", "bp_eval_mix", "bp_score_waves_ext", "bp_eval_mix_ext", "bp_eval_mix_logmmse_ext",
    "bp_stream_open", "bp_stream_push", "bp_stream_close", "bp_stream_counts", "bp_stream_packed",
    "bp_logmmse_defaults", "bp_logmmse_waves", "bp_eval_mix_logmmse",
    "bp_lmstream_open", "bp_lmstream_push", "bp_lmstream_close", "bp_lmstream_counts",
    "bp_noise_defaults", "bp_logmmse_waves_nt", "bp_eval_mix_logmmse_nt", "bp_lmstream_open_nt", "bp_set_nat",
    "bp_resample_defaults", "bp_resample_ratio", "bp_resample_len", "bp_resample_taps", "bp_resample_waves",
    "bp_mel_defaults", "bp_mel_filters", "bp_mel_dct", "bp_wave_mfcc", "bp_set_mix_aux",
    "bp_post_defaults", "bp_set_post", "bp_post_rows", "bp_gv_mix", "bp_gv_factors",
    "bp_rbm_defaults", "bp_rbm_create", "bp_rbm_destroy", "bp_rbm_set_hyper", "bp_rbm_train_chunk", "bp_rbm_up", "bp_rbm_step",
    "bp_rbm_steps", "bp_rbm_get",
]
WAVE_LPS, WAVE_MASK = 0, 1      # bp_wave_chunk.target
FORWARD_DEFAULT, FORWARD_ROWINV = 0, 1   # bp_set_forward
NAT_STATIC, NAT_DYNAMIC = 0, 1           # bp_set_nat
NAT_MODES = {"static": NAT_STATIC, "dynamic": NAT_DYNAMIC}
GV_RAW, GV_POST = 0, 1                   # bp_gv_mix: stage
GV_STAGES = {"raw": GV_RAW, "post": GV_POST}
GV_INDEP, GV_DEP = 0, 1                  # bp_gv_factors: mode
GV_MODES = {"indep": GV_INDEP, "dep": GV_DEP}
MIX_LPS, MIX_IRM, MIX_IBM, MIX_LPS_IRM, MIX_LPS_IBM = 0, 1, 2, 3, 4   # bp_mix_corpus.target
SCORE_SSNR, SCORE_LSD, SCORE_STOI = 0, 1, 2   # columns of bp_score_waves / bp_eval_mix scores
SCORE_ESTOI, SCORE_SISDR = 3, 4               # the two further columns of the _ext calls (extended=True)
REVERB_TARGET_REVERBERANT, REVERB_TARGET_EARLY = 0, 1   # bp_mix_reverb.target
REVERB_TARGETS = {"reverberant": REVERB_TARGET_REVERBERANT, "early": REVERB_TARGET_EARLY}
MIX_RIR_MAX_TAPS = 65536
RIR_MAX_IMAGES = 1 << 26
# bp_rir_room: a numpy structured array of this dtype is a list of rooms
RIR_ROOM_DTYPE = np.dtype([("L", np.float64, 3), ("src", np.float64, 3), ("mic", np.float64, 3), ("beta", np.float64, 6)])
# bp_rir_range: the defaults of rir_rooms (and of bpmix / bpeval)
RIR_RANGE_DEFAULTS = dict(L_lo=(3.0, 3.0, 2.5), L_hi=(10.0, 8.0, 4.0), t60=(0.2, 0.8), margin=0.5, dist=(0.5, 3.0))
MIX_TARGETS = {"lps": MIX_LPS, "irm": MIX_IRM, "ibm": MIX_IBM, "lps+irm": MIX_LPS_IRM, "lps+ibm": MIX_LPS_IBM}
# bp_mixture: a numpy structured array of this dtype is a mixture plan
MIXTURE_DTYPE = np.dtype({"names": ["clean", "noise", "offset", "snr_db"], "formats": [np.int32, np.int32, np.int64, np.float32],
                          "offsets": [0, 4, 8, 16], "itemsize": 24})
PROF_KINDS = ["fwd_l1", "fwd_hidden", "fwd_out", "dgrad_out", "dgrad_hidden", "wgrad_update_grouped"]


class BPError(RuntimeError):
    pass


class BPWindowChunk(C.Structure):
    """bp_window_chunk (include/bp_c_api.h): raw frames + index tables, stacked on the device."""
    _fields_ = [
        ("n_samples", C.c_int), ("n_frames", C.c_int), ("fea_dim", C.c_int), ("context", C.c_int), ("n_nat", C.c_int),
        ("fea", C.POINTER(C.c_float)), ("targ_frames", C.POINTER(C.c_float)), ("nat", C.POINTER(C.c_float)),
        ("win_start", C.POINTER(C.c_int)), ("targ_frame", C.POINTER(C.c_int)), ("nat_row", C.POINTER(C.c_int)),
    ]


class BPWaveChunk(C.Structure):
    """bp_wave_chunk (include/bp_c_api.h): noisy sentences for bp_enhance_waves."""
    _fields_ = [
        ("n_sent", C.c_int), ("sent_len", C.POINTER(C.c_int)), ("pcm", C.POINTER(C.c_float)),
        ("context", C.c_int), ("targ_offset", C.c_int),
        ("mean", C.POINTER(C.c_float)), ("inv_std", C.POINTER(C.c_float)),
        ("target", C.c_int), ("out_col", C.c_int),
    ]


class BPMixCorpus(C.Structure):
    """bp_mix_corpus (include/bp_c_api.h): clean and noise recordings, resident on the handle."""
    _fields_ = [
        ("fea_dim", C.c_int), ("context", C.c_int), ("targ_offset", C.c_int), ("target", C.c_int), ("lc_db", C.c_float),
        ("mean", C.POINTER(C.c_float)), ("inv_std", C.POINTER(C.c_float)),
        ("n_clean", C.c_int), ("clean_len", C.POINTER(C.c_int64)), ("clean_pcm", C.POINTER(C.c_float)),
        ("n_noise", C.c_int), ("noise_len", C.POINTER(C.c_int64)), ("noise_pcm", C.POINTER(C.c_float)),
    ]


class BPMixReverb(C.Structure):
    """bp_mix_reverb (include/bp_c_api.h): impulse responses and the {clean, response} pairs that become derived entries."""
    _fields_ = [
        ("n_rir", C.c_int), ("rir_len", C.POINTER(C.c_int)), ("rir_pcm", C.POINTER(C.c_float)),
        ("n_pair", C.c_int), ("pair_clean", C.POINTER(C.c_int)), ("pair_rir", C.POINTER(C.c_int)),
        ("target", C.c_int), ("early_taps", C.c_int),
    ]


class BPRirRange(C.Structure):
    """bp_rir_range (include/bp_c_api.h): the ranges bp_rir_rooms draws rooms from."""
    _fields_ = [
        ("L_lo", C.c_double * 3), ("L_hi", C.c_double * 3), ("t60_lo", C.c_double), ("t60_hi", C.c_double),
        ("margin", C.c_double), ("dist_lo", C.c_double), ("dist_hi", C.c_double),
    ]


class BPStreamConfig(C.Structure):
    """bp_stream_config (include/bp_c_api.h): a streaming session of n_chan channels."""
    _fields_ = [
        ("fea_dim", C.c_int), ("context", C.c_int), ("targ_offset", C.c_int),
        ("mean", C.POINTER(C.c_float)), ("inv_std", C.POINTER(C.c_float)),
        ("target", C.c_int), ("out_col", C.c_int), ("n_chan", C.c_int), ("max_push_samples", C.c_int),
    ]


class BPLogmmseParams(C.Structure):
    """bp_logmmse_params (include/bp_c_api.h): the log-MMSE baseline's parameters."""
    _fields_ = [
        ("alpha", C.c_double), ("mu", C.c_double), ("eta", C.c_double), ("xi_min_db", C.c_double), ("gamma_max", C.c_double),
        ("init_frames", C.c_int),
    ]


class BPNoiseParams(C.Structure):
    """bp_noise_params (include/bp_c_api.h): the noise update of the log-MMSE baseline."""
    _fields_ = [
        ("mode", C.c_int), ("xi_h1_db", C.c_double), ("q", C.c_double), ("a_pow", C.c_double), ("a_spp", C.c_double),
        ("p_lo", C.c_double), ("p_cap", C.c_double),
    ]


NOISE_VAD, NOISE_SPP = 0, 1


class BPResampleParams(C.Structure):
    """bp_resample_params (include/bp_c_api.h): the windowed-sinc filter of the sample-rate converter."""
    _fields_ = [("zeros", C.c_int), ("beta", C.c_double), ("rolloff", C.c_double)]


class BPMelParams(C.Structure):
    """bp_mel_params (include/bp_c_api.h): the MFCC auxiliary target.  mean / scale point into arrays the owner keeps alive
    (mel_params stores them on the object)."""
    _fields_ = [
        ("sample_rate", C.c_int), ("n_mel", C.c_int), ("n_ceps", C.c_int), ("first_coef", C.c_int),
        ("f_lo", C.c_float), ("f_hi", C.c_float), ("lifter", C.c_float),
        ("mean", C.POINTER(C.c_float)), ("scale", C.POINTER(C.c_float)),
    ]


class BPPostParams(C.Structure):
    """bp_post_params (include/bp_c_api.h): post-processing of the LPS estimate.  gv_center / gv_scale point into arrays the owner
    keeps alive (post_params stores them on the object)."""
    _fields_ = [
        ("gv", C.c_int), ("gv_center", C.POINTER(C.c_float)), ("gv_scale", C.POINTER(C.c_float)),
        ("mask_col", C.c_int), ("mask_lo", C.c_float), ("mask_hi", C.c_float), ("mask_weight", C.c_float),
    ]


class BPRbmConfig(C.Structure):
    """bp_rbm_config (include/bp_c_api.h): a stack of RBMs."""
    _fields_ = [
        ("device", C.c_int), ("numlayers", C.c_int), ("layersizes", C.c_int * MAXLAYER),
        ("bunchsize", C.c_int), ("max_chunk_frames", C.c_int), ("seed", C.c_uint64),
    ]


class BPRbmHyper(C.Structure):
    """bp_rbm_hyper (include/bp_c_api.h): the hyper-parameters of one RBM's CD-1 step."""
    _fields_ = [("lrate", C.c_float), ("momentum", C.c_float), ("weightcost", C.c_float), ("visible", C.c_int), ("sample", C.c_int)]


class BPRbmTrace(C.Structure):
    """bp_rbm_trace (include/bp_c_api.h): what bp_rbm_step hands back; any pointer may be NULL."""
    _fields_ = [
        ("v0", C.POINTER(C.c_float)), ("p0", C.POINTER(C.c_float)), ("s0", C.POINTER(C.c_float)), ("v1", C.POINTER(C.c_float)),
        ("p1", C.POINTER(C.c_float)), ("gw", C.POINTER(C.c_float)), ("gc", C.POINTER(C.c_float)), ("ga", C.POINTER(C.c_float)),
        ("recon", C.POINTER(C.c_double)),
    ]


class BPConfig(C.Structure):
    _fields_ = [
        ("gpu_used", C.c_int), ("numlayers", C.c_int), ("layersizes", C.c_int * MAXLAYER),
        ("bunchsize", C.c_int), ("lrate", C.c_float), ("momentum", C.c_float), ("weightcost", C.c_float),
        ("dropoutflag", C.c_int), ("visible_omit", C.c_float), ("hid_omit", C.c_float),
        ("activation", C.c_int), ("momentum_rule", C.c_int), ("seed", C.c_uint64), ("device", C.c_int),
        ("global_bunchsize", C.c_int), ("rank_frame_offset", C.c_int), ("max_chunk_frames", C.c_int),
        ("compute_dtype", C.c_int),
    ]


_lib = None


def load_library(path=None):
    """dlopen the HIP library (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("BP_HIP_LIB", LIB_PATH)   # (BP_HIP_LIB: development builds of the same ABI)
    if not os.path.exists(p):
        raise BPError("HIP library %s not found: build it with `python __graft_entry__.py` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback" % p)
    lib = C.CDLL(p)
    fpp = C.POINTER(C.POINTER(C.c_float))
    fp = C.POINTER(C.c_float)
    hp = C.c_void_p
    lib.bp_last_error.restype = C.c_char_p
    lib.bp_build_target.restype = C.c_char_p
    lib.bp_create.argtypes = [C.POINTER(BPConfig), fpp, fpp, C.POINTER(hp)]
    lib.bp_destroy.argtypes = [hp]
    lib.bp_train_chunk.argtypes = [hp, C.c_int, fp, fp]
    lib.bp_cv_chunk.argtypes = [hp, C.c_int, fp, fp, fp]
    lib.bp_forward.argtypes = [hp, C.c_int, fp, fp]
    lib.bp_get_weights.argtypes = [hp, fpp, fpp]
    lib.bp_get_deltas.argtypes = [hp, fpp, fpp]
    lib.bp_upload_chunk.argtypes = [hp, C.c_int, fp, fp]
    lib.bp_upload_chunk_windows.argtypes = [hp, C.POINTER(BPWindowChunk)]
    lib.bp_train_chunk_windows.argtypes = [hp, C.POINTER(BPWindowChunk)]
    lib.bp_cv_chunk_windows.argtypes = [hp, C.POINTER(BPWindowChunk), fp]
    lib.bp_forward_windows.argtypes = [hp, C.POINTER(BPWindowChunk), fp]
    lib.bp_enhance_waves.argtypes = [hp, C.c_int, C.POINTER(BPWaveChunk), fp, fp]
    lib.bp_wave_lps.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), fp, fp]
    lib.bp_set_mix_corpus.argtypes = [hp, C.POINTER(BPMixCorpus)]
    lib.bp_train_mix.argtypes = [hp, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    lib.bp_cv_mix.argtypes = [hp, C.c_int, C.c_void_p, fp]
    lib.bp_mix_features.argtypes = [hp, C.c_int, C.c_void_p, fp, fp, fp, fp, fp]
    lib.bp_mix_plan.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int, fp, C.c_void_p]
    lib.bp_mix_shuffle.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_int)]
    ip = C.POINTER(C.c_int)
    lib.bp_set_mix_reverb.argtypes = [hp, C.POINTER(BPMixReverb)]
    lib.bp_reverb_waves.argtypes = [C.c_int, C.c_int, ip, fp, ip, C.c_int, ip, fp, C.c_int, fp, fp]
    lib.bp_mix_rir_delay.argtypes = [fp, C.c_int, ip]
    lib.bp_mix_reverb_pairs.argtypes = [C.c_uint64, C.c_int, C.c_int, ip]
    dp = C.POINTER(C.c_double)
    lib.bp_rir_image.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, ip, fp]
    lib.bp_rir_orders.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ip, C.POINTER(C.c_int64)]
    lib.bp_rir_beta.argtypes = [dp, C.c_double, dp]
    lib.bp_rir_rooms.argtypes = [C.c_uint64, C.c_int, C.POINTER(BPRirRange), C.c_void_p]
    lib.bp_score_waves.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), fp, fp, fp]
    lib.bp_eval_mix.argtypes = [hp, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, fp, fp, fp]
    lib.bp_score_waves_ext.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), fp, fp, C.c_int, fp]
    lib.bp_eval_mix_ext.argtypes = [hp, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, fp]
    lib.bp_eval_mix_logmmse_ext.argtypes = [hp, C.POINTER(BPLogmmseParams), C.c_int, C.c_void_p, C.c_int, C.c_int, fp, fp, fp]
    lib.bp_logmmse_defaults.argtypes = [C.POINTER(BPLogmmseParams)]
    lib.bp_logmmse_waves.argtypes = [C.c_int, C.c_int, C.POINTER(BPLogmmseParams), C.c_int, C.POINTER(C.c_int), fp, fp, fp, fp]
    lib.bp_eval_mix_logmmse.argtypes = [hp, C.POINTER(BPLogmmseParams), C.c_int, C.c_void_p, C.c_int, fp, fp, fp]
    lib.bp_stream_open.argtypes = [hp, C.POINTER(BPStreamConfig), C.POINTER(C.c_void_p)]
    lib.bp_stream_push.argtypes = [C.c_void_p, C.POINTER(C.c_int), fp, C.POINTER(C.c_ubyte), C.POINTER(C.c_int), fp, C.c_size_t]
    lib.bp_stream_close.argtypes = [C.c_void_p]
    lib.bp_stream_counts.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int] + [C.POINTER(C.c_int64)] * 3
    lib.bp_lmstream_open.argtypes = [C.c_int, C.c_int, C.POINTER(BPLogmmseParams), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.bp_lmstream_push.argtypes = [C.c_void_p, C.POINTER(C.c_int), fp, C.POINTER(C.c_ubyte), C.POINTER(C.c_int), fp, C.c_size_t]
    lib.bp_lmstream_close.argtypes = [C.c_void_p]
    lib.bp_noise_defaults.argtypes = [C.POINTER(BPNoiseParams)]
    lib.bp_logmmse_waves_nt.argtypes = [C.c_int, C.c_int, C.POINTER(BPLogmmseParams), C.POINTER(BPNoiseParams), C.c_int, C.POINTER(C.c_int),
                                        fp, fp, fp, fp, fp]
    lib.bp_eval_mix_logmmse_nt.argtypes = [hp, C.POINTER(BPLogmmseParams), C.POINTER(BPNoiseParams), C.c_int, C.c_void_p, C.c_int, C.c_int,
                                           fp, fp, fp]
    lib.bp_lmstream_open_nt.argtypes = [C.c_int, C.c_int, C.POINTER(BPLogmmseParams), C.POINTER(BPNoiseParams), C.c_int, C.c_int,
                                        C.POINTER(C.c_void_p)]
    lib.bp_lmstream_counts.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int] + [C.POINTER(C.c_int64)] * 3
    lib.bp_resample_defaults.argtypes = [C.POINTER(BPResampleParams)]
    lib.bp_resample_ratio.argtypes = [C.c_int, C.c_int, ip, ip]
    lib.bp_resample_len.argtypes = [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    lib.bp_resample_taps.argtypes = [C.c_int, C.c_int, C.POINTER(BPResampleParams), fp, C.c_int]
    lib.bp_resample_waves.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(BPResampleParams), C.c_int, ip, fp, fp]
    lib.bp_fill_chunk_synthetic.argtypes = [hp, C.c_int, C.c_uint64]
    lib.bp_train_resident.argtypes = [hp, C.c_int, C.c_int]
    lib.bp_sync.argtypes = [hp]
    lib.bp_grads_resident.argtypes = [hp, C.c_int]
    lib.bp_grad_floats.argtypes = [hp, C.POINTER(C.c_size_t)]
    lib.bp_read_grads.argtypes = [hp, fp, C.c_size_t]
    lib.bp_grad_layout.argtypes = [hp, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.bp_last_train_ms.argtypes = [hp, fp, C.POINTER(C.c_int)]
    lib.bp_time_kernel.argtypes = [hp, C.c_int, C.c_int, fp]
    lib.bp_train_resident_masked.argtypes = [hp, C.c_int, C.c_int, C.POINTER(C.POINTER(C.c_uint8))]
    lib.bp_profile_step.argtypes = [hp, C.c_int, C.c_int, fp, C.POINTER(C.c_int)]
    lib.bp_measure_peaks.argtypes = [hp, fp, fp]
    lib.bp_set_hyper.argtypes = [hp, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
    lib.bp_set_output.argtypes = [hp, C.c_int, C.c_int, C.c_int]
    lib.bp_set_forward.argtypes = [hp, C.c_int]
    lib.bp_set_nat.argtypes = [hp, C.c_int, C.POINTER(BPNoiseParams)]
    ip = C.POINTER(C.c_int)
    lib.bp_mel_defaults.argtypes = [C.c_int, C.POINTER(BPMelParams)]
    lib.bp_mel_filters.argtypes = [C.c_int, C.POINTER(BPMelParams), fp, ip, ip]
    lib.bp_mel_dct.argtypes = [C.POINTER(BPMelParams), fp]
    lib.bp_wave_mfcc.argtypes = [C.c_int, C.c_int, C.POINTER(BPMelParams), C.c_int, ip, fp, fp, fp, fp]
    lib.bp_set_mix_aux.argtypes = [hp, C.POINTER(BPMelParams)]
    lib.bp_stream_packed.argtypes = [C.c_void_p]
    lib.bp_post_defaults.argtypes = [C.POINTER(BPPostParams)]
    lib.bp_set_post.argtypes = [hp, C.c_int, C.POINTER(BPPostParams)]
    lib.bp_post_rows.argtypes = [C.c_int, C.c_int, C.c_int, fp, fp, fp, C.POINTER(BPPostParams), fp]
    lib.bp_gv_mix.argtypes = [hp, C.c_int, C.c_void_p, C.c_int, C.c_int, dp, dp, dp, dp, C.POINTER(C.c_int64)]
    lib.bp_gv_factors.argtypes = [C.c_int, C.c_int64, dp, dp, dp, dp, C.c_int, fp, fp]
    lib.bp_rbm_defaults.argtypes = [C.c_int, C.POINTER(BPRbmHyper)]
    lib.bp_rbm_create.argtypes = [C.POINTER(BPRbmConfig), fpp, fpp, fpp, C.POINTER(C.c_void_p)]
    lib.bp_rbm_destroy.argtypes = [C.c_void_p]
    lib.bp_rbm_set_hyper.argtypes = [C.c_void_p, C.c_int, C.POINTER(BPRbmHyper)]
    lib.bp_rbm_train_chunk.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, dp]
    lib.bp_rbm_up.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, fp]
    lib.bp_rbm_step.argtypes = [C.c_void_p, C.c_int, fp, C.c_int, C.POINTER(BPRbmTrace)]
    lib.bp_rbm_steps.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint)]
    lib.bp_rbm_get.argtypes = [C.c_void_p, fpp, fpp, fpp]
    lib.bp_dp_attach.argtypes = [hp, C.c_int, C.c_int, C.c_char_p]
    lib.bp_dp_attach_ex.argtypes = [hp, C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.bp_dp_peer_info.argtypes = [hp, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.bp_dp_handoff.argtypes = [hp, C.POINTER(C.c_int)]
    lib.bp_dp_barrier.argtypes = [hp]
    lib.bp_dp_allgather.argtypes = [hp, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.bp_rdv_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]
    lib.bp_rdv_barrier.argtypes = [C.c_void_p]
    lib.bp_rdv_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.bp_rdv_close.argtypes = [C.c_void_p]
    lib.bp_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
    lib.bp_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.bp_host_register.argtypes = [C.c_void_p, C.c_size_t]
    lib.bp_host_unregister.argtypes = [C.c_void_p]
    lib.bp_read_layer_output.argtypes = [hp, C.c_int, fp, C.c_size_t]
    lib.bp_dp_detach.argtypes = [hp]
    lib.bp_dp_info.argtypes = [hp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
    if path is None:
        _lib = lib
    return lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ptrs(arrs):
    P = C.POINTER(C.c_float)
    out = (P * MAXLAYER)()
    for i, a in enumerate(arrs):
        if a is not None:
            out[i] = a.ctypes.data_as(P)
    return out


class BP_GPU(object):
    """Drop-in for the reference trainer object; see module docstring."""

    def __init__(self, gpu_used, numlayers, layersizes, bunchsize, lrate, momentum, weightcost, weights, bias,
                 dropoutflag=0, visible_omit=0.0, hid_omit=0.0, activation=0, momentum_rule=0, seed=0, device=0,
                 global_bunchsize=0, rank_frame_offset=0, max_chunk_frames=0, strict_exit=False, compute_dtype=0,
                 output_activation=0, output_linear_cols=0, output_loss=0, forward_mode=FORWARD_DEFAULT, nat_mode="static",
                 nat_noise=None):
        self._h = None
        self._strict = strict_exit
        self._lib = load_library()
        self.numlayers = int(numlayers)
        self.layersizes = [int(x) for x in list(layersizes)[:numlayers]]
        self.bunchsize = int(bunchsize)
        self.lrate, self.momentum, self.weightcost = float(lrate), float(momentum), float(weightcost)
        self.dropoutflag, self.visible_omit, self.hid_omit = int(dropoutflag), float(visible_omit), float(hid_omit)
        cfg = BPConfig()
        cfg.gpu_used, cfg.numlayers, cfg.bunchsize = int(gpu_used), self.numlayers, self.bunchsize
        for i, s in enumerate(self.layersizes[:MAXLAYER]):
            cfg.layersizes[i] = s
        cfg.lrate, cfg.momentum, cfg.weightcost = self.lrate, self.momentum, self.weightcost
        cfg.dropoutflag, cfg.visible_omit, cfg.hid_omit = self.dropoutflag, self.visible_omit, self.hid_omit
        cfg.activation, cfg.momentum_rule, cfg.seed, cfg.device = int(activation), int(momentum_rule), int(seed), int(device)
        cfg.global_bunchsize, cfg.rank_frame_offset = int(global_bunchsize), int(rank_frame_offset)
        cfg.max_chunk_frames = int(max_chunk_frames)
        cfg.compute_dtype = int(compute_dtype)          # 0 fp32 (reference) | 1 bf16 operands, fp32 accumulate / master weights
        self._cfg = cfg
        if len(self.layersizes) != self.numlayers or self.numlayers < 2 or self.numlayers > MAXLAYER - 1:
            self._fail("numlayers must be in 2..%d and match layersizes" % (MAXLAYER - 1))
        w = [None] * MAXLAYER
        b = [None] * MAXLAYER
        for l in range(1, self.numlayers):
            w[l] = np.ascontiguousarray(weights[l], dtype=np.float32).reshape(-1)
            b[l] = np.ascontiguousarray(bias[l], dtype=np.float32).reshape(-1)
            if w[l].size != self.layersizes[l - 1] * self.layersizes[l] or b[l].size != self.layersizes[l]:
                self._fail("weights[%d]/bias[%d] have the wrong size" % (l, l))
        out_mode = self._output_args(output_activation, output_linear_cols, output_loss)
        self.output_activation = self.output_linear_cols = self.output_loss = 0
        h = C.c_void_p()
        self._check(self._lib.bp_create(C.byref(cfg), _ptrs(w), _ptrs(b), C.byref(h)))
        self._h = h
        self.forward_mode = FORWARD_DEFAULT
        if out_mode != (0, 0, 0):
            self.set_output(*out_mode)
        if int(forward_mode) != FORWARD_DEFAULT:
            self.set_forward(forward_mode)
        self._nat_mode = "static"
        self._mix_aux = self._mix_aux_set = None
        if nat_mode != "static" or nat_noise is not None:
            self.set_nat(nat_mode, nat_noise)

    # ------------------------------------------------------------------ errors
    def _fail(self, msg):
        if self._strict:                      # reference convention: printf + exit(0)
            print(msg)
            sys.exit(0)
        raise BPError(msg)

    def _check(self, rc):
        if rc != 0:
            self._fail("%s (status %d)" % (self._lib.bp_last_error().decode(), rc))

    def _in(self, a, n_frames, width, name):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.size < n_frames * width:
            self._fail("%s holds %d floats, need %d" % (name, a.size, n_frames * width))
        return a

    # ------------------------------------------------------------------ reference API
    def _push_hyper(self):
        """The reference reads its public members afresh on every bunch (BP_GPU.cu:488-500): a caller may
        assign obj.lrate / momentum / weightcost / dropoutflag / visible_omit / hid_omit between chunks.  Every method that runs
        the net pushes them first -- training, CV and gradients, and also the forwards (forward, enhance_waves, eval_mix, a
        stream's push: the keep-scale follows dropoutflag and the omit rates) -- so that what a call computes does not depend
        on which method was called before it."""
        self._check(self._lib.bp_set_hyper(self._h, float(self.lrate), float(self.momentum), float(self.weightcost),
                                           int(self.dropoutflag), float(self.visible_omit), float(self.hid_omit)))

    def _output_args(self, activation, linear_cols, loss):
        """Checks of bp_set_output, made here so that a bad value never reaches the library."""
        a, c, s = int(activation), int(linear_cols), int(loss)
        if a not in (0, 1):
            self._fail("output activation must be 0 (linear) or 1 (logistic)")
        if s not in (0, 1):
            self._fail("output loss must be 0 (cross-entropy) or 1 (squared error)")
        if a == 0 and (c != 0 or s != 0):
            self._fail("output linear_cols and loss must be 0 with the linear output")
        if a == 1 and not 0 <= c < self.layersizes[-1]:
            self._fail("output linear_cols must be in [0, %d) with the logistic output" % self.layersizes[-1])
        return a, c, s

    def set_output(self, activation, linear_cols=0, loss=0):
        """Output-layer nonlinearity (bp_set_output): 0 linear; 1 logistic on the output columns [linear_cols, sL), trained
        with loss 0 (cross-entropy: dEdz = 2/Bg (y - t)) or 1 (squared error through the logistic).  From the next call on."""
        a, c, s = self._output_args(activation, linear_cols, loss)
        self._check(self._lib.bp_set_output(self._h, a, c, s))
        self.output_activation, self.output_linear_cols, self.output_loss = a, c, s

    def set_forward(self, mode):
        """The kernels of the inference forward (bp_set_forward): FORWARD_DEFAULT, or FORWARD_ROWINV -- a frame's output bits then
        depend on its input row and the net alone, and streams opened from now on pack their channels.  fp32 handles."""
        self._check(self._lib.bp_set_forward(self._h, int(mode)))
        self.forward_mode = int(mode)

    def set_nat(self, mode, noise=None):
        """The noise-aware block of the calls that stage it (bp_set_nat): "static", one row per sentence (the default), or
        "dynamic", one row per frame from the MMSE-SPP noise tracker -- enhance_waves, train_mix, CrossValid_mix, mix_features
        and eval_mix from the next call on, and the streams opened from now on (an open stream keeps its mode).  noise: what noise_params takes (None: the tracker's defaults)."""
        if mode not in NAT_MODES:
            self._fail("set_nat: mode must be \"static\" or \"dynamic\", not %r" % (mode,))
        try:
            nz = noise_params(noise)
        except BPError as e:
            self._fail(str(e))
        self._check(self._lib.bp_set_nat(self._h, NAT_MODES[mode], C.byref(nz)))
        self._nat_mode = mode

    @property
    def nat_mode(self):
        """"static" or "dynamic": what set_nat (or nat_mode= at construction) set last."""
        return self._nat_mode

    def set_post(self, gv_center=None, gv_scale=None, mask_col=-1, mask_lo=0.5, mask_hi=0.5, mask_weight=1.0, fea_dim=None):
        """Post-processing of the LPS estimate before resynthesis (bp_set_post): GV equalisation x = c + s (x - c) with gv_center and
        gv_scale (what gv_factors returns), then the mask gate -- the noisy LPS blended in where the mask columns from mask_col on say
        that speech dominates.  enhance_waves and eval_mix from the next call on, and the streams opened from now on.  set_post(None),
        or no argument at all, switches it off.  fea_dim: needed only for gating without GV (default: the corpus's)."""
        if gv_center is None and gv_scale is None and int(mask_col) < 0:
            self._check(self._lib.bp_set_post(self._h, 0, None))
            self._post = False
            return
        try:
            p = post_params(gv_center, gv_scale, mask_col, mask_lo, mask_hi, mask_weight)
        except BPError as e:
            self._fail(str(e))
        D = p._center.size if p.gv else fea_dim if fea_dim is not None else getattr(self, "mix_fea_dim", None)
        if D is None:
            self._fail("set_post: fea_dim is needed for gating without GV on a handle without a corpus")
        self._check(self._lib.bp_set_post(self._h, int(D), C.byref(p)))
        self._post = True

    @property
    def post(self):
        """True while post-processing is on (set_post)."""
        return getattr(self, "_post", False)

    def gv_mix(self, plan, out_col=0, stage="raw"):
        """bp_gv_mix: the second moments the GV factors are made from, over the plan's mixtures: dict of est_sum, est_sq, ref_sum,
        ref_sq (float64 [fea_dim]) and frames.  stage "raw": the net's columns from out_col on; "post": the rows that are
        resynthesised (set_post).  Across plans the caller adds the sums; gv_factors takes the dict."""
        if stage not in GV_STAGES:
            self._fail("gv_mix: stage must be \"raw\" or \"post\", not %r" % (stage,))
        p, pp = self._plan(plan)
        self._push_hyper()
        D = getattr(self, "mix_fea_dim", None) or 1
        out = {k: np.zeros(D, np.float64) for k in ("est_sum", "est_sq", "ref_sum", "ref_sq")}
        n = C.c_int64(0)
        dpt = C.POINTER(C.c_double)
        self._check(self._lib.bp_gv_mix(self._h, p.size, pp, int(out_col), GV_STAGES[stage], out["est_sum"].ctypes.data_as(dpt),
                                        out["est_sq"].ctypes.data_as(dpt), out["ref_sum"].ctypes.data_as(dpt),
                                        out["ref_sq"].ctypes.data_as(dpt), C.byref(n)))
        out["frames"] = int(n.value)
        return out

    def set_mix_aux(self, mel):
        """The MFCC auxiliary target of the mixing corpus (bp_set_mix_aux): what mel_params makes, or None for none.  From the next
        set_mix_corpus on -- its target must then begin with LPS and layersizes[-1] be parts * fea_dim + n_ceps; the target row is
        [LPS | MFCC | mask].  A corpus that is already set keeps what it was set with."""
        if mel is not None and not isinstance(mel, BPMelParams):
            self._fail("set_mix_aux: mel must be None or what mel_params returns")
        self._check(self._lib.bp_set_mix_aux(self._h, None if mel is None else C.byref(mel)))
        self._mix_aux = None if mel is None else (int(mel.n_mel), int(mel.n_ceps))

    @property
    def mix_aux_dims(self):
        """(n_mel, n_ceps) of the MFCC columns of the corpus set last, or None when it has none."""
        return self._mix_aux_set

    def train(self, n_frames, indata, targ):
        x = self._in(indata, n_frames, self.layersizes[0], "in")
        t = self._in(targ, n_frames, self.layersizes[-1], "targ")
        self._push_hyper()
        self._check(self._lib.bp_train_chunk(self._h, int(n_frames), _fp(x), _fp(t)))

    def CrossValid(self, n_frames, indata, targ):
        x = self._in(indata, n_frames, self.layersizes[0], "in")
        t = self._in(targ, n_frames, self.layersizes[-1], "targ")
        self._push_hyper()
        e = C.c_float(0.0)
        self._check(self._lib.bp_cv_chunk(self._h, int(n_frames), _fp(x), _fp(t), C.byref(e)))
        return float(e.value)

    def returnWeights(self, weights, bias):
        """Fills caller-owned arrays weights[l]/bias[l], l = 1..numlayers-1 (index 0 unused)."""
        for l in range(1, self.numlayers):
            for a, n in ((weights[l], self.layersizes[l - 1] * self.layersizes[l]), (bias[l], self.layersizes[l])):
                if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.size == n):
                    self._fail("returnWeights: arrays must be contiguous float32 of the layer's size")
        self._check(self._lib.bp_get_weights(self._h, _ptrs(weights), _ptrs(bias)))

    # ------------------------------------------------------------------ conveniences / extensions
    def _new_params(self):
        w = [None] + [np.empty((self.layersizes[l - 1], self.layersizes[l]), np.float32) for l in range(1, self.numlayers)]
        b = [None] + [np.empty(self.layersizes[l], np.float32) for l in range(1, self.numlayers)]
        return w, b

    def get_weights(self):
        w, b = self._new_params()
        self.returnWeights(w, b)
        return w, b

    def get_deltas(self):
        w, b = self._new_params()
        self._check(self._lib.bp_get_deltas(self._h, _ptrs(w), _ptrs(b)))
        return w, b

    def forward(self, indata):
        x = np.ascontiguousarray(indata, dtype=np.float32).reshape(-1, self.layersizes[0])
        out = np.empty((x.shape[0], self.layersizes[-1]), np.float32)
        self._push_hyper()
        self._check(self._lib.bp_forward(self._h, x.shape[0], _fp(x), _fp(out)))
        return out

    def upload_chunk(self, indata, targ):
        x = np.ascontiguousarray(indata, dtype=np.float32).reshape(-1, self.layersizes[0])
        t = self._in(targ, x.shape[0], self.layersizes[-1], "targ")
        self._check(self._lib.bp_upload_chunk(self._h, x.shape[0], _fp(x), _fp(t)))

    # ---- on-device frame stacking (bp_window_chunk): sample i = fea[win_start[i] : win_start[i]+context] (+ nat[nat_row[i]])
    def _windows(self, fea, targ_frames, context, win_start, targ_frame, nat=None, nat_row=None):
        fea = np.ascontiguousarray(fea, dtype=np.float32)
        if fea.ndim != 2:
            self._fail("windows: fea must be [n_frames][fea_dim]")
        tg = np.ascontiguousarray(targ_frames, dtype=np.float32).reshape(fea.shape[0], self.layersizes[-1])
        ws = np.ascontiguousarray(win_start, dtype=np.int32)
        tf = np.ascontiguousarray(targ_frame, dtype=np.int32)
        c = BPWindowChunk()
        c.n_samples, c.n_frames, c.fea_dim, c.context = int(ws.size), int(fea.shape[0]), int(fea.shape[1]), int(context)
        c.fea, c.targ_frames = _fp(fea), _fp(tg)
        ip = C.POINTER(C.c_int)
        c.win_start, c.targ_frame = ws.ctypes.data_as(ip), tf.ctypes.data_as(ip)
        keep = [fea, tg, ws, tf]
        if nat is not None:
            nat = np.ascontiguousarray(nat, dtype=np.float32).reshape(-1, fea.shape[1])
            nr = np.ascontiguousarray(nat_row, dtype=np.int32)
            c.n_nat, c.nat, c.nat_row = int(nat.shape[0]), _fp(nat), nr.ctypes.data_as(ip)
            keep += [nat, nr]
        return c, keep

    def upload_chunk_windows(self, fea, targ_frames, context, win_start, targ_frame, nat=None, nat_row=None):
        c, keep = self._windows(fea, targ_frames, context, win_start, targ_frame, nat, nat_row)
        self._check(self._lib.bp_upload_chunk_windows(self._h, C.byref(c)))

    def train_windows(self, fea, targ_frames, context, win_start, targ_frame, nat=None, nat_row=None):
        c, keep = self._windows(fea, targ_frames, context, win_start, targ_frame, nat, nat_row)
        self._push_hyper()
        self._check(self._lib.bp_train_chunk_windows(self._h, C.byref(c)))

    def CrossValid_windows(self, fea, targ_frames, context, win_start, targ_frame, nat=None, nat_row=None):
        c, keep = self._windows(fea, targ_frames, context, win_start, targ_frame, nat, nat_row)
        e = C.c_float(0.0)
        self._push_hyper()
        self._check(self._lib.bp_cv_chunk_windows(self._h, C.byref(c), C.byref(e)))
        return float(e.value)

    # ---- waveform enhancement (bp_enhance_waves; signal definition: include/bp_c_api.h)
    def enhance_waves(self, sentences, mean, inv_std, context, targ_offset, target=WAVE_LPS, out_col=0, return_net=False):
        """Noisy sentences (1-D float32, int16 units) -> enhanced sentences of the same lengths; with return_net also the
        net outputs per frame, one [T_s][layersizes[-1]] array per sentence."""
        mean = np.ascontiguousarray(mean, dtype=np.float32).reshape(-1)
        inv_std = np.ascontiguousarray(inv_std, dtype=np.float32).reshape(-1)
        D = mean.size
        if inv_std.size != D:
            self._fail("enhance_waves: mean and inv_std differ in length")
        pcm, lens, frames = _sentences(sentences, D)
        c = BPWaveChunk()
        c.n_sent, c.sent_len, c.pcm = len(lens), lens.ctypes.data_as(C.POINTER(C.c_int)), _fp(pcm)
        c.context, c.targ_offset, c.mean, c.inv_std = int(context), int(targ_offset), _fp(mean), _fp(inv_std)
        c.target, c.out_col = int(target), int(out_col)
        out = np.empty(max(pcm.size, 1), np.float32)
        net = np.empty((max(int(frames.sum()), 1), self.layersizes[-1]), np.float32) if return_net else None
        self._push_hyper()
        self._check(self._lib.bp_enhance_waves(self._h, D, C.byref(c), _fp(out), _fp(net) if return_net else None))
        waves = np.split(out[:pcm.size], np.cumsum(lens)[:-1])
        if not return_net:
            return waves
        return waves, np.split(net[:int(frames.sum())], np.cumsum(frames)[:-1])

    # ---- streaming sessions (bp_stream_open ...; contract: include/bp_c_api.h)
    def stream_open(self, mean, inv_std, context, targ_offset, target=WAVE_LPS, out_col=0, n_chan=1, max_push_samples=16000):
        """A Stream of n_chan channels on this handle: push(blocks, end) returns the samples that became final, the same bits as
        enhance_waves on the finished sentences.  Close it (or the handle) when done."""
        mean = np.ascontiguousarray(mean, dtype=np.float32).reshape(-1)
        inv_std = np.ascontiguousarray(inv_std, dtype=np.float32).reshape(-1)
        if inv_std.size != mean.size:
            self._fail("stream_open: mean and inv_std differ in length")
        c = BPStreamConfig()
        c.fea_dim, c.context, c.targ_offset, c.mean, c.inv_std = mean.size, int(context), int(targ_offset), _fp(mean), _fp(inv_std)
        c.target, c.out_col, c.n_chan, c.max_push_samples = int(target), int(out_col), int(n_chan), int(max_push_samples)
        s = C.c_void_p()
        self._check(self._lib.bp_stream_open(self._h, C.byref(c), C.byref(s)))
        return Stream(self, s, mean.size, int(context), int(targ_offset), int(n_chan), bool(self._lib.bp_stream_packed(s)),
                      self._nat_mode, self.post)

    # ---- training mixtures made on the device (bp_set_mix_corpus ...; definition: include/bp_c_api.h)
    def set_mix_corpus(self, clean, noise, mean, inv_std, context, targ_offset, target=MIX_LPS, lc_db=5.0):
        """clean, noise: lists of 1-D arrays (int16 units), uploaded once; target: MIX_* or a name of MIX_TARGETS."""
        mean = np.ascontiguousarray(mean, dtype=np.float32).reshape(-1)
        inv_std = np.ascontiguousarray(inv_std, dtype=np.float32).reshape(-1)
        if inv_std.size != mean.size:
            self._fail("set_mix_corpus: mean and inv_std differ in length")
        target = MIX_TARGETS[target] if isinstance(target, str) else int(target)
        cl = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in clean]
        no = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in noise]
        cpcm = np.ascontiguousarray(np.concatenate(cl) if cl else np.zeros(0, np.float32))
        npcm = np.ascontiguousarray(np.concatenate(no) if no else np.zeros(0, np.float32))
        clen = np.array([x.size for x in cl], np.int64)
        nlen = np.array([x.size for x in no], np.int64)
        c = BPMixCorpus()
        c.fea_dim, c.context, c.targ_offset, c.target, c.lc_db = mean.size, int(context), int(targ_offset), target, float(lc_db)
        c.mean, c.inv_std = _fp(mean), _fp(inv_std)
        lp = C.POINTER(C.c_int64)
        c.n_clean, c.clean_len, c.clean_pcm = len(cl), clen.ctypes.data_as(lp), _fp(cpcm)
        c.n_noise, c.noise_len, c.noise_pcm = len(no), nlen.ctypes.data_as(lp), _fp(npcm)
        self._check(self._lib.bp_set_mix_corpus(self._h, C.byref(c)))
        self.mix_fea_dim, self.mix_clean_len = mean.size, clen
        self.mix_nat = self.layersizes[0] == (int(context) + 1) * mean.size
        self.mix_n_clean, self.mix_reverb_entries = len(cl), 0
        self._mix_aux_set = self._mix_aux

    def set_mix_reverb(self, rirs, pair_clean, pair_rir, target="reverberant", early_taps=0):
        """bp_set_mix_reverb: pair k = (clean sentence pair_clean[k], response rirs[pair_rir[k]]) becomes clean entry n_clean + k
        of the corpus; target: "reverberant" | "early" (REVERB_TARGETS) or the number; replaces the entries of an earlier call."""
        target = REVERB_TARGETS[target] if isinstance(target, str) else int(target)
        hs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in rirs]
        hlen = np.array([x.size for x in hs], np.int32)
        hpcm = np.ascontiguousarray(np.concatenate(hs) if hs else np.zeros(0, np.float32))
        pc = np.ascontiguousarray(pair_clean, dtype=np.int32).reshape(-1)
        pr = np.ascontiguousarray(pair_rir, dtype=np.int32).reshape(-1)
        if pc.size != pr.size:
            self._fail("set_mix_reverb: pair_clean and pair_rir differ in length")
        ip = C.POINTER(C.c_int)
        r = BPMixReverb()
        r.n_rir, r.rir_len, r.rir_pcm = len(hs), hlen.ctypes.data_as(ip), _fp(hpcm)
        r.n_pair, r.pair_clean, r.pair_rir = pc.size, pc.ctypes.data_as(ip), pr.ctypes.data_as(ip)
        r.target, r.early_taps = target, int(early_taps)
        self._check(self._lib.bp_set_mix_reverb(self._h, C.byref(r)))
        n = self.mix_n_clean
        self.mix_clean_len = np.concatenate([self.mix_clean_len[:n], self.mix_clean_len[:n][pc]])
        self.mix_reverb_entries = int(pc.size)

    def _plan(self, plan):
        p = np.ascontiguousarray(plan, dtype=MIXTURE_DTYPE).reshape(-1)
        return p, p.ctypes.data_as(C.c_void_p)

    def mix_frames(self, plan):
        """Frames of every mixture of the plan (T = (len_c - 1)/hop + 2), per the corpus set last."""
        p = np.ascontiguousarray(plan, dtype=MIXTURE_DTYPE).reshape(-1)
        if getattr(self, "mix_fea_dim", None) is None:
            self._fail("mix_frames: no corpus (set_mix_corpus)")
        lens = self.mix_clean_len[p["clean"]]
        return (lens - 1) // (self.mix_fea_dim - 1) + 2

    def train_mix(self, plan, order=None):
        p, pp = self._plan(plan)
        self._push_hyper()
        o = None if order is None else np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        if o is not None and o.size != int(self.mix_frames(p).sum()):     # (the library reads sum(T) entries)
            self._fail("train_mix: order must have one entry per frame of the plan (%d), not %d" % (int(self.mix_frames(p).sum()), o.size))
        self._check(self._lib.bp_train_mix(self._h, p.size, pp, None if o is None else o.ctypes.data_as(C.POINTER(C.c_int))))

    def CrossValid_mix(self, plan):
        p, pp = self._plan(plan)
        self._push_hyper()
        e = C.c_float(0.0)
        self._check(self._lib.bp_cv_mix(self._h, p.size, pp, C.byref(e)))
        return float(e.value)

    def mix_features(self, plan):
        """dict of fea [sum T][D] (normalised), lps [sum T][D] (noisy), targ [sum T][sL], nat [n_mix][D] (None without the
        noise-aware block; in nat_mode "dynamic" [sum T][D], the row of every frame) and pcm [sum len_c] (the mixed samples),
        unshuffled."""
        p, pp = self._plan(plan)
        D = getattr(self, "mix_fea_dim", None)
        if D is None:                                   # no corpus: the library reports the state error
            self._check(self._lib.bp_mix_features(self._h, p.size, pp, None, None, None, None, None))
        T = int(self.mix_frames(p).sum())
        n_pcm = int(self.mix_clean_len[p["clean"]].sum())
        has_nat = self.mix_nat
        out = {"fea": np.empty((T, D), np.float32), "lps": np.empty((T, D), np.float32),
               "targ": np.empty((T, self.layersizes[-1]), np.float32),
               "nat": np.empty((T if self._nat_mode == "dynamic" else p.size, D), np.float32) if has_nat else None, "pcm": np.empty(max(n_pcm, 1), np.float32)}
        self._check(self._lib.bp_mix_features(self._h, p.size, pp, _fp(out["fea"]), _fp(out["lps"]), _fp(out["targ"]),
                                              _fp(out["nat"]) if has_nat else None, _fp(out["pcm"])))
        out["pcm"] = out["pcm"][:n_pcm]
        return out

    def eval_mix(self, plan, sample_rate, target=WAVE_LPS, out_col=0, return_pcm=False, extended=False):
        """bp_eval_mix: the plan's mixtures made on the device, enhanced with this net and scored against their clean sentences.
        dict of noisy [n_mix][3] and enhanced [n_mix][3] float32 scores (columns SCORE_SSNR, SCORE_LSD, SCORE_STOI; NaN where
        undefined) and pcm: the enhanced sentences (a list) with return_pcm, else None.  extended: bp_eval_mix_ext with five
        columns, SCORE_ESTOI and SCORE_SISDR behind the same three."""
        p, pp = self._plan(plan)
        self._push_hyper()
        ns = 5 if extended else 3
        noisy = np.empty((max(p.size, 1), ns), np.float32)
        enh = np.empty((max(p.size, 1), ns), np.float32)
        pcm = None
        if return_pcm and getattr(self, "mix_fea_dim", None) is not None:
            lens = self.mix_clean_len[p["clean"]] if p.size else np.zeros(0, np.int64)
            pcm = np.empty(max(int(lens.sum()), 1), np.float32)
        if extended:
            self._check(self._lib.bp_eval_mix_ext(self._h, p.size, pp, int(sample_rate), int(target), int(out_col), ns, _fp(noisy),
                                                  _fp(enh), _fp(pcm) if pcm is not None else None))
        else:
            self._check(self._lib.bp_eval_mix(self._h, p.size, pp, int(sample_rate), int(target), int(out_col), _fp(noisy), _fp(enh),
                                              _fp(pcm) if pcm is not None else None))
        if pcm is not None:
            pcm = np.split(pcm[:int(lens.sum())], np.cumsum(lens)[:-1])
        return {"noisy": noisy[:p.size], "enhanced": enh[:p.size], "pcm": pcm}

    def eval_mix_logmmse(self, plan, sample_rate, params=None, return_pcm=False, extended=False, noise=None):
        """bp_eval_mix_logmmse: eval_mix with the log-MMSE baseline in place of the net (params: None for the defaults, a dict of
        bp_logmmse_params fields over them, or a BPLogmmseParams).  The same dictionary as eval_mix (extended: five columns,
        bp_eval_mix_logmmse_ext).  noise: as for logmmse_waves (anything but None: bp_eval_mix_logmmse_nt)."""
        p, pp = self._plan(plan)
        ns = 5 if extended else 3
        noisy = np.empty((max(p.size, 1), ns), np.float32)
        enh = np.empty((max(p.size, 1), ns), np.float32)
        pcm = None
        if return_pcm and getattr(self, "mix_fea_dim", None) is not None:
            lens = self.mix_clean_len[p["clean"]] if p.size else np.zeros(0, np.int64)
            pcm = np.empty(max(int(lens.sum()), 1), np.float32)
        lm = logmmse_params(params)
        lmp = None if lm is None else C.byref(lm)
        if noise is not None:
            nz = noise_params(noise)
            self._check(self._lib.bp_eval_mix_logmmse_nt(self._h, lmp, C.byref(nz), p.size, pp, int(sample_rate), ns, _fp(noisy), _fp(enh),
                                                         _fp(pcm) if pcm is not None else None))
        elif extended:
            self._check(self._lib.bp_eval_mix_logmmse_ext(self._h, lmp, p.size, pp, int(sample_rate), ns, _fp(noisy), _fp(enh),
                                                          _fp(pcm) if pcm is not None else None))
        else:
            self._check(self._lib.bp_eval_mix_logmmse(self._h, lmp, p.size, pp, int(sample_rate), _fp(noisy), _fp(enh),
                                                      _fp(pcm) if pcm is not None else None))
        if pcm is not None:
            pcm = np.split(pcm[:int(lens.sum())], np.cumsum(lens)[:-1])
        return {"noisy": noisy[:p.size], "enhanced": enh[:p.size], "pcm": pcm}

    def fill_chunk_synthetic(self, n_frames, seed=20260927):
        self._check(self._lib.bp_fill_chunk_synthetic(self._h, int(n_frames), int(seed)))

    def train_resident(self, first_frame, n_frames):
        self._push_hyper()
        self._check(self._lib.bp_train_resident(self._h, int(first_frame), int(n_frames)))

    def train_resident_masked(self, first_frame, n_frames, masks):
        """masks[l], l = 0..numlayers-2: uint8 [n_frames][layersizes[l]] (1 = drop) or None -- parity tests only."""
        P = C.POINTER(C.c_uint8)
        arr = (P * MAXLAYER)()
        keep = []
        for l, m in enumerate(masks):
            if m is not None:
                m = np.ascontiguousarray(m, dtype=np.uint8).reshape(int(n_frames), self.layersizes[l])
                keep.append(m)
                arr[l] = m.ctypes.data_as(P)
        self._push_hyper()
        self._check(self._lib.bp_train_resident_masked(self._h, int(first_frame), int(n_frames), arr))

    # ---- gradients without the update (parity tests): bp_grads_resident / bp_read_grads / bp_read_layer_output
    def grads_resident(self, first_frame):
        self._push_hyper()
        self._check(self._lib.bp_grads_resident(self._h, int(first_frame)))

    def grad_floats(self):
        n = C.c_size_t()
        self._check(self._lib.bp_grad_floats(self._h, C.byref(n)))
        return n.value

    def grad_layout(self, layer):
        o, c = C.c_size_t(), C.c_size_t()
        self._check(self._lib.bp_grad_layout(self._h, int(layer), C.byref(o), C.byref(c)))
        return o.value, c.value

    def read_grads(self, padded=False):
        """Per-layer weight / bias gradients of the last bp_grads_resident, unpadded: ([None, G_1 [prev][cur], ...], [None, gb_1, ...]).
        padded: the layers as they lie in the flat buffer (bp_grad_layout), widths rounded up to 64, pad rows and columns included."""
        g = np.empty(self.grad_floats(), np.float32)
        self._check(self._lib.bp_read_grads(self._h, _fp(g), g.size))
        pad = lambda v: (v + 63) & ~63
        gw, gb = [None], [None]
        for l in range(1, self.numlayers):
            off, cnt = self.grad_layout(l)
            lp, lc = pad(self.layersizes[l - 1]), pad(self.layersizes[l])
            assert cnt == lp * lc + lc
            rows, cols = (lp, lc) if padded else (self.layersizes[l - 1], self.layersizes[l])
            gw.append(g[off:off + lp * lc].reshape(lp, lc)[:rows, :cols].copy())
            gb.append(g[off + lp * lc:off + cnt][:cols].copy())
        return gw, gb

    def read_layer_output(self, layer):
        y = np.empty((self.bunchsize, self.layersizes[layer]), np.float32)
        self._check(self._lib.bp_read_layer_output(self._h, int(layer), _fp(y), y.size))
        return y

    # ---- in-library data-parallel exchange (bp_dp_attach, include/bp_c_api.h)
    def dp_attach(self, world, rank, key, transport=0):
        """transport: 0 = the library's peer kernels over hipIpc mappings (reduce-scatter by peer reads), 1 = RCCL reduce-scatter /
        all-gather, 2 = the library's peer kernels in push form (every rank writes its slices into the owners' receive buffers)."""
        self._check(self._lib.bp_dp_attach_ex(self._h, int(world), int(rank), str(key).encode(), int(transport)))

    def dp_peer_info(self, peer):
        """(device ordinal in the peer's process, PCI bus id, transport, acquire mode) of rank `peer`."""
        dev, tr, aq = C.c_int(), C.c_int(), C.c_int()
        buf = C.create_string_buffer(32)
        self._check(self._lib.bp_dp_peer_info(self._h, int(peer), C.byref(dev), buf, 32, C.byref(tr), C.byref(aq)))
        return int(dev.value), buf.value.decode(), int(tr.value), int(aq.value)

    def dp_handoff(self):
        """True: gradient segments are handed to the exchange inside the running weight-gradient launch (tile counters);
        False: event + kernel boundary per group of layers."""
        v = C.c_int()
        self._check(self._lib.bp_dp_handoff(self._h, C.byref(v)))
        return bool(v.value)

    def dp_barrier(self):
        self._check(self._lib.bp_dp_barrier(self._h))

    def dp_allgather_f64(self, value, world):
        mine = (C.c_double * 1)(float(value))
        out = (C.c_double * int(world))()
        self._check(self._lib.bp_dp_allgather(self._h, mine, 8, out))
        return [float(v) for v in out]

    def dp_detach(self):
        self._check(self._lib.bp_dp_detach(self._h))

    def dp_info(self):
        w, r, n = C.c_int(), C.c_int(), C.c_uint()
        self._check(self._lib.bp_dp_info(self._h, C.byref(w), C.byref(r), C.byref(n)))
        return int(w.value), int(r.value), int(n.value)

    def sync(self):
        self._check(self._lib.bp_sync(self._h))

    def last_train_ms(self):
        ms, nb = C.c_float(), C.c_int()
        self._check(self._lib.bp_last_train_ms(self._h, C.byref(ms), C.byref(nb)))
        return float(ms.value), int(nb.value)

    def time_kernel(self, which, iters=50):
        ms = C.c_float()
        self._check(self._lib.bp_time_kernel(self._h, int(which), int(iters), C.byref(ms)))
        return float(ms.value)

    def profile_step(self, first_frame, n_bunches):
        """{class: (avg ms per launch inside the step, launches per step)} -- bp_profile_step."""
        ms = (C.c_float * len(PROF_KINDS))()
        cnt = (C.c_int * len(PROF_KINDS))()
        self._push_hyper()
        self._check(self._lib.bp_profile_step(self._h, int(first_frame), int(n_bunches), ms, cnt))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(PROF_KINDS)}

    def measure_peaks(self):
        a, b = C.c_float(), C.c_float()
        self._check(self._lib.bp_measure_peaks(self._h, C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def close(self):
        if self._h is not None:
            self._lib.bp_destroy(self._h)       # (releases the handle's open streams too)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stream_push(lib_call, handle, n_chan, blocks, end, out_cap):
    """One push of either kind of stream (bp_stream_push, bp_lmstream_push): (status, one float32 array per channel or None).
    out_cap: samples of the output buffer, or a function of the samples pushed that gives them."""
    arrs = [np.zeros(0, np.float32) if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in blocks]
    n_in = np.array([a.size for a in arrs], np.int32)
    pcm = np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros(0, np.float32)
    e = None if end is None else np.ascontiguousarray([1 if v else 0 for v in end], dtype=np.uint8)
    if callable(out_cap):
        out_cap = out_cap(int(pcm.size))
    out = np.empty(max(int(out_cap), 1), np.float32)
    n_out = np.zeros(n_chan, np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib_call(handle, n_in.ctypes.data_as(ip), _fp(pcm) if pcm.size else None,
                  None if e is None else e.ctypes.data_as(C.POINTER(C.c_ubyte)), n_out.ctypes.data_as(ip), _fp(out), int(out_cap))
    return rc, None if rc != 0 else [a.copy() for a in np.split(out[:int(n_out.sum())], np.cumsum(n_out)[:-1])]


def _counts3(fn, *args):
    """(frames_in, frames_out, samples_out) from the count call named fn (bp_stream_counts, bp_lmstream_counts); host only."""
    lib = load_library()
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    rc = getattr(lib, fn)(*(args + (C.byref(a), C.byref(b), C.byref(c))))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return int(a.value), int(b.value), int(c.value)


class Stream(object):
    """A streaming session (bp_stream_*): n_chan live feeds enhanced in blocks of any sizes."""

    def __init__(self, owner, s, fea_dim, context, targ_offset, n_chan, packed=False, nat_mode="static", post=False):
        self._g, self._s, self._packed, self._nat_mode, self._post = owner, s, bool(packed), nat_mode, bool(post)
        self.fea_dim, self.context, self.targ_offset, self.n_chan = fea_dim, context, targ_offset, n_chan
        self.look_ahead = context - 1 - targ_offset

    @property
    def packed(self):
        """True for a stream opened in FORWARD_ROWINV: a push places its frames densely and runs the row-invariant forward, whatever
        the handle's mode is by then."""
        return self._packed

    @property
    def nat_mode(self):
        """"static" or "dynamic": the noise-aware block the stream stages -- its handle's mode (set_nat) when it was opened,
        whatever the handle's mode is by then."""
        return self._nat_mode

    @property
    def post(self):
        """True for a stream opened with post-processing on (set_post): it keeps the parameters its handle had then."""
        return self._post

    def push(self, blocks, end=None, out_cap=None):
        """blocks: one 1-D array of new samples per channel (None or empty: none); end: per channel, true closes the channel's
        sentence after these samples.  Returns one float32 array per channel: the samples that became final.  out_cap: size of
        the output buffer in samples (default: everything a push of this size can return)."""
        g = self._g
        if self._s is None or g._h is None:
            g._fail("Stream.push: the stream or its handle is closed")
        if len(blocks) != self.n_chan or (end is not None and len(end) != self.n_chan):
            g._fail("Stream.push: need one block (and one end flag) per channel (%d)" % self.n_chan)
        if out_cap is None:     # what waited (at most max(look-ahead, 5) + 1 frames) and what arrived, rounded up to frames
            out_cap = lambda n: n + self.n_chan * (max(self.look_ahead, 5) + 3) * (self.fea_dim - 1)
        g._push_hyper()
        rc, outs = _stream_push(g._lib.bp_stream_push, self._s, self.n_chan, blocks, end, out_cap)
        g._check(rc)
        return outs

    def close(self):
        if self._s is not None and self._g._h is not None:
            self._g._lib.bp_stream_close(self._s)
        self._s = None


def stream_counts(fea_dim, context, targ_offset, nat, received, ended):
    """bp_stream_counts: (frames_in, frames_out, samples_out) of a channel after `received` samples of its sentence; host only."""
    return _counts3("bp_stream_counts", int(fea_dim), int(context), int(targ_offset), 1 if nat else 0, int(received),
                    1 if ended else 0)


def _sentences(sentences, fea_dim):
    """Concatenated float32 samples, int32 lengths and the frame count of every sentence (T = (n-1)/hop + 2)."""
    arrs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in sentences]
    lens = np.array([a.size for a in arrs], np.int32)
    pcm = np.concatenate(arrs) if arrs else np.zeros(0, np.float32)
    hop = max(fea_dim - 1, 1)
    frames = np.where(lens > 0, (lens - 1) // hop + 2, 0).astype(np.int64)
    return np.ascontiguousarray(pcm), lens, frames


def wave_lps(device, fea_dim, sentences):
    """bp_wave_lps: the log-power spectrum of every sentence, one [T_s][fea_dim] float32 array each (no handle)."""
    lib = load_library()
    pcm, lens, frames = _sentences(sentences, int(fea_dim))
    out = np.empty((max(int(frames.sum()), 1), int(fea_dim)), np.float32)
    rc = lib.bp_wave_lps(int(device), int(fea_dim), len(lens), lens.ctypes.data_as(C.POINTER(C.c_int)), _fp(pcm), _fp(out))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return np.split(out[:int(frames.sum())], np.cumsum(frames)[:-1])


def post_params(gv_center=None, gv_scale=None, mask_col=-1, mask_lo=0.5, mask_hi=0.5, mask_weight=1.0):
    """A BPPostParams over bp_post_defaults: GV on when gv_center and gv_scale are given (both or neither)."""
    lib = load_library()
    p = BPPostParams()
    lib.bp_post_defaults(C.byref(p))
    if (gv_center is None) != (gv_scale is None):
        raise BPError("post_params: gv_center and gv_scale come together")
    if gv_center is not None:
        p._center = np.ascontiguousarray(gv_center, dtype=np.float32).reshape(-1)
        p._scale = np.ascontiguousarray(gv_scale, dtype=np.float32).reshape(-1)
        if p._center.size != p._scale.size:
            raise BPError("post_params: gv_center and gv_scale differ in length")
        p.gv, p.gv_center, p.gv_scale = 1, _fp(p._center), _fp(p._scale)
    p.mask_col, p.mask_lo, p.mask_hi, p.mask_weight = int(mask_col), float(mask_lo), float(mask_hi), float(mask_weight)
    return p


def post_rows(device, est, noisy_lps, mask=None, gv_center=None, gv_scale=None, mask_lo=0.5, mask_hi=0.5, mask_weight=1.0):
    """bp_post_rows: the post-processed value over rows [n_frames][fea_dim] (no handle): GV with gv_center / gv_scale when given,
    the gate when a mask block is given."""
    lib = load_library()
    est = np.ascontiguousarray(est, dtype=np.float32)
    y = np.ascontiguousarray(noisy_lps, dtype=np.float32)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
    if est.ndim != 2 or y.shape != est.shape or (m is not None and m.shape != est.shape):
        raise BPError("post_rows: est, noisy_lps and mask must be [n_frames][fea_dim] arrays of one shape")
    p = post_params(gv_center, gv_scale, 0 if m is not None else -1, mask_lo, mask_hi, mask_weight)
    if p.gv and p._center.size != est.shape[1]:
        raise BPError("post_rows: gv_center and gv_scale must have fea_dim entries")
    out = np.empty(est.shape if est.size else (1, 1), np.float32)
    rc = lib.bp_post_rows(int(device), est.shape[1], est.shape[0], _fp(est), None if m is None else _fp(m), _fp(y), C.byref(p), _fp(out))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return out


def gv_factors(stats, mode="indep"):
    """bp_gv_factors (host only): (center, scale), float32 [fea_dim], from the sums of gv_mix (a dict; sums of several calls added
    by the caller).  mode "indep": one factor for all bins, "dep": one per bin."""
    lib = load_library()
    if mode not in GV_MODES:
        raise BPError("gv_factors: mode must be \"indep\" or \"dep\", not %r" % (mode,))
    s = [np.ascontiguousarray(stats[k], dtype=np.float64).reshape(-1) for k in ("est_sum", "est_sq", "ref_sum", "ref_sq")]
    D = s[0].size
    if any(a.size != D for a in s):
        raise BPError("gv_factors: the four sums differ in length")
    center, scale = np.empty(max(D, 1), np.float32), np.empty(max(D, 1), np.float32)
    dpt = C.POINTER(C.c_double)
    rc = lib.bp_gv_factors(D, int(stats["frames"]), *[a.ctypes.data_as(dpt) for a in s], GV_MODES[mode], _fp(center), _fp(scale))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return center[:D], scale[:D]


def mel_params(sample_rate, **fields):
    """A BPMelParams: bp_mel_defaults(sample_rate) -- 26 filters, 13 coefficients from c0, 0 .. sample_rate / 2, lifter 22, no mean
    or scale -- overridden by the fields given (n_mel, n_ceps, first_coef, f_lo, f_hi, lifter; mean, scale: n_ceps values each).  A
    weight alpha_r on coefficient r's squared error is scale_r * sqrt(alpha_r)."""
    lib = load_library()
    mp = BPMelParams()
    rc = lib.bp_mel_defaults(int(sample_rate), C.byref(mp))
    if rc != 0:
        _raise(lib, rc)
    names = [f[0] for f in BPMelParams._fields_]
    for k, v in fields.items():
        if k not in names or k == "sample_rate":
            raise BPError("mel_params: unknown field %s" % k)
        if k in ("mean", "scale"):
            continue
        setattr(mp, k, float(v) if k in ("f_lo", "f_hi", "lifter") else int(v))
    for k in ("mean", "scale"):
        if fields.get(k) is not None:
            a = np.ascontiguousarray(fields[k], dtype=np.float32).reshape(-1)
            if a.size != mp.n_ceps:
                raise BPError("mel_params: %s must hold n_ceps = %d values, not %d" % (k, mp.n_ceps, a.size))
            setattr(mp, "_keep_" + k, a)                    # (the struct holds a pointer into it)
            setattr(mp, k, _fp(a))
    return mp


def mel_filters(fea_dim, mel):
    """bp_mel_filters: (w [n_mel][fea_dim] float32, first_bin [n_mel], n_bins [n_mel]) -- the triangles and the bins with w > 0; host only."""
    lib = load_library()
    n = max(int(mel.n_mel), 0)
    w = np.zeros((n, max(int(fea_dim), 1)), np.float32)
    first, nb = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    ip = C.POINTER(C.c_int)
    rc = lib.bp_mel_filters(int(fea_dim), C.byref(mel), _fp(w) if w.size else None, first.ctypes.data_as(ip), nb.ctypes.data_as(ip))
    if rc != 0:
        _raise(lib, rc)
    return w, first[:n], nb[:n]


def mel_dct(mel):
    """bp_mel_dct: t [n_ceps][n_mel] float32, the liftered DCT-II rows first_coef .. first_coef + n_ceps - 1; host only."""
    lib = load_library()
    n, c = max(int(mel.n_mel), 0), max(int(mel.n_ceps), 0)
    t = np.zeros((c, n), np.float32)
    rc = lib.bp_mel_dct(C.byref(mel), _fp(t) if t.size else None)
    if rc != 0:
        _raise(lib, rc)
    return t


def wave_mfcc(device, fea_dim, sentences, mel, return_logmel=False, return_power=False):
    """bp_wave_mfcc: the MFCC target rows of every sentence, one [T_s][n_ceps] float32 array each (mean and scale applied; no
    handle).  With return_logmel / return_power a dict of mfcc and logmel [T_s][n_mel] / power [T_s][fea_dim] lists."""
    lib = load_library()
    pcm, lens, frames = _sentences(sentences, int(fea_dim))
    T = int(frames.sum())
    n_mel, n_ceps = max(int(mel.n_mel), 1), max(int(mel.n_ceps), 1)
    cc = np.empty((max(T, 1), n_ceps), np.float32)
    lm = np.empty((max(T, 1), n_mel), np.float32) if return_logmel else None
    pw = np.empty((max(T, 1), int(fea_dim)), np.float32) if return_power else None
    rc = lib.bp_wave_mfcc(int(device), int(fea_dim), C.byref(mel), len(lens), lens.ctypes.data_as(C.POINTER(C.c_int)), _fp(pcm),
                          None if pw is None else _fp(pw), None if lm is None else _fp(lm), _fp(cc))
    if rc != 0:
        _raise(lib, rc)
    cut = np.cumsum(frames)[:-1]
    out = {"mfcc": np.split(cc[:T], cut)}
    if not return_logmel and not return_power:
        return out["mfcc"]
    if return_logmel:
        out["logmel"] = np.split(lm[:T], cut)
    if return_power:
        out["power"] = np.split(pw[:T], cut)
    return out


def logmmse_params(params=None):
    """None (the library's defaults), or a BPLogmmseParams: bp_logmmse_defaults overridden by the fields of a dict."""
    if params is None or isinstance(params, BPLogmmseParams):
        return params
    lib = load_library()
    lm = BPLogmmseParams()
    lib.bp_logmmse_defaults(C.byref(lm))
    names = [f[0] for f in BPLogmmseParams._fields_]
    for k, v in dict(params).items():
        if k not in names:
            raise BPError("logmmse_params: unknown field %s" % k)
        setattr(lm, k, int(v) if k == "init_frames" else float(v))
    return lm


def noise_params(noise=None):
    """A BPNoiseParams: bp_noise_defaults (the MMSE-SPP tracker) for None or "spp", the VAD-gated update for "vad", the defaults
    overridden by the fields of a dict (mode: 0 / 1 or "vad" / "spp"), or the BPNoiseParams given."""
    if isinstance(noise, BPNoiseParams):
        return noise
    lib = load_library()
    nz = BPNoiseParams()
    lib.bp_noise_defaults(C.byref(nz))
    modes = {"vad": NOISE_VAD, "spp": NOISE_SPP}
    if noise is None:
        return nz
    if isinstance(noise, str):
        noise = {"mode": noise}
    names = [f[0] for f in BPNoiseParams._fields_]
    for k, v in dict(noise).items():
        if k not in names:
            raise BPError("noise_params: unknown field %s" % k)
        if k == "mode":
            if isinstance(v, str) and v not in modes:
                raise BPError("noise_params: unknown mode %s" % v)
            nz.mode = modes[v] if isinstance(v, str) else int(v)
        else:
            setattr(nz, k, float(v))
    return nz


def logmmse_waves(device, fea_dim, sentences, params=None, return_gain=False, return_vad=False, noise=None, return_noise=False):
    """bp_logmmse_waves: every sentence enhanced by the log-MMSE baseline (no handle, no net): a list of float32 arrays, or with
    return_gain / return_vad / return_noise a tuple (pcm, gain [T_s][fea_dim] per sentence, vad [T_s] per sentence, noise
    [T_s][fea_dim] per sentence; the ones not asked for omitted).  noise: None for the call as it always was, else "spp", "vad",
    a dict of bp_noise_params fields or a BPNoiseParams (noise_params): bp_logmmse_waves_nt.  return_noise needs the latter call
    and, with noise None, makes it in VAD mode: the same bits, and the lambda every frame's gamma used."""
    lib = load_library()
    pcm, lens, frames = _sentences(sentences, int(fea_dim))
    T = int(frames.sum())
    out = np.empty(max(pcm.size, 1), np.float32)
    gain = np.empty((max(T, 1), int(fea_dim)), np.float32) if return_gain else None
    vad = np.empty(max(T, 1), np.float32) if return_vad else None
    nse = np.empty((max(T, 1), int(fea_dim)), np.float32) if return_noise else None
    lm = logmmse_params(params)
    if noise is None and not return_noise:
        rc = lib.bp_logmmse_waves(int(device), int(fea_dim), None if lm is None else C.byref(lm), len(lens),
                                  lens.ctypes.data_as(C.POINTER(C.c_int)), _fp(pcm), _fp(out), None if gain is None else _fp(gain),
                                  None if vad is None else _fp(vad))
    else:
        nz = noise_params("vad" if noise is None else noise)
        rc = lib.bp_logmmse_waves_nt(int(device), int(fea_dim), None if lm is None else C.byref(lm), C.byref(nz), len(lens),
                                     lens.ctypes.data_as(C.POINTER(C.c_int)), _fp(pcm), _fp(out), None if gain is None else _fp(gain),
                                     None if vad is None else _fp(vad), None if nse is None else _fp(nse))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    res = [np.split(out[:pcm.size], np.cumsum(lens)[:-1])]
    if return_gain:
        res.append(np.split(gain[:T], np.cumsum(frames)[:-1]))
    if return_vad:
        res.append(np.split(vad[:T], np.cumsum(frames)[:-1]))
    if return_noise:
        res.append(np.split(nse[:T], np.cumsum(frames)[:-1]))
    return res[0] if len(res) == 1 else tuple(res)


class LogmmseStream(object):
    """A log-MMSE stream (bp_lmstream_*): n_chan live feeds enhanced by the classic baseline in blocks of any sizes; no handle."""

    def __init__(self, lib, s, fea_dim, init_frames, n_chan):
        self._lib, self._s = lib, s
        self.fea_dim, self.init_frames, self.n_chan = fea_dim, init_frames, n_chan

    def push(self, blocks, end=None, out_cap=None):
        """blocks: one 1-D array of new samples per channel (None or empty: none); end: per channel, true closes the channel's
        sentence after these samples.  Returns one float32 array per channel: the samples that became final.  out_cap: size of
        the output buffer in samples (default: everything a push of this size can return)."""
        if self._s is None:
            raise BPError("LogmmseStream.push: the stream is closed")
        if len(blocks) != self.n_chan or (end is not None and len(end) != self.n_chan):
            raise BPError("LogmmseStream.push: need one block (and one end flag) per channel (%d)" % self.n_chan)
        if out_cap is None:     # what waited for the noise start (fewer than init_frames + 1 hops) and what arrived
            out_cap = lambda n: n + self.n_chan * (self.init_frames + 1) * (self.fea_dim - 1)
        rc, outs = _stream_push(self._lib.bp_lmstream_push, self._s, self.n_chan, blocks, end, out_cap)
        if rc != 0:
            raise BPError("%s (status %d)" % (self._lib.bp_last_error().decode(), rc))
        return outs

    def close(self):
        if self._s is not None:
            self._lib.bp_lmstream_close(self._s)
        self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def logmmse_stream_open(device, fea_dim, params=None, n_chan=1, max_push_samples=16000, noise=None):
    """bp_lmstream_open: a LogmmseStream of n_chan channels on a device ordinal (params and noise as for logmmse_waves; noise
    other than None: bp_lmstream_open_nt)."""
    lib = load_library()
    lm = logmmse_params(params)
    s = C.c_void_p()
    lmp = None if lm is None else C.byref(lm)
    if noise is None:
        rc = lib.bp_lmstream_open(int(device), int(fea_dim), lmp, int(n_chan), int(max_push_samples), C.byref(s))
    else:
        nz = noise_params(noise)
        rc = lib.bp_lmstream_open_nt(int(device), int(fea_dim), lmp, C.byref(nz), int(n_chan), int(max_push_samples), C.byref(s))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    if lm is None:
        lm = BPLogmmseParams()
        lib.bp_logmmse_defaults(C.byref(lm))
    return LogmmseStream(lib, s, int(fea_dim), int(lm.init_frames), int(n_chan))


def logmmse_stream_counts(fea_dim, init_frames, received, ended):
    """bp_lmstream_counts: (frames_in, frames_out, samples_out) of a channel after `received` samples of its sentence; host only."""
    return _counts3("bp_lmstream_counts", int(fea_dim), int(init_frames), int(received), 1 if ended else 0)


def score_waves(device, fea_dim, sample_rate, refs, ests, extended=False):
    """bp_score_waves: SSNR, LSD and STOI of every estimate against its reference (lists of 1-D arrays, int16 units, pairwise
    equal lengths), float32 [n][3] (columns SCORE_SSNR, SCORE_LSD, SCORE_STOI; NaN where undefined).  No handle.  extended:
    bp_score_waves_ext, float32 [n][5] with SCORE_ESTOI and SCORE_SISDR behind the same three."""
    lib = load_library()
    if len(refs) != len(ests):
        raise BPError("score_waves: %d references but %d estimates" % (len(refs), len(ests)))
    r = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in refs]
    e = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in ests]
    for k, (a, b) in enumerate(zip(r, e)):
        if a.size != b.size:
            raise BPError("score_waves: pair %d: reference has %d samples, estimate %d" % (k, a.size, b.size))
    lens = np.array([a.size for a in r], np.int32)
    rp = np.ascontiguousarray(np.concatenate(r) if r else np.zeros(0, np.float32))
    ep = np.ascontiguousarray(np.concatenate(e) if e else np.zeros(0, np.float32))
    out = np.empty((max(len(r), 1), 5 if extended else 3), np.float32)
    lp = lens.ctypes.data_as(C.POINTER(C.c_int))
    if extended:
        rc = lib.bp_score_waves_ext(int(device), int(fea_dim), int(sample_rate), len(r), lp, _fp(rp), _fp(ep), 5, _fp(out))
    else:
        rc = lib.bp_score_waves(int(device), int(fea_dim), int(sample_rate), len(r), lp, _fp(rp), _fp(ep), _fp(out))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return out[:len(r)]


def _raise(lib, rc):
    raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))


def resample_params(params=None):
    """None (the library's defaults: zeros 16, beta 8.6, rolloff 0.9), or a BPResampleParams: bp_resample_defaults overridden by
    the fields of a dict, or by a (zeros, beta, rolloff) tuple."""
    if params is None or isinstance(params, BPResampleParams):
        return params
    lib = load_library()
    rs = BPResampleParams()
    lib.bp_resample_defaults(C.byref(rs))
    if not isinstance(params, dict):
        params = dict(zip(("zeros", "beta", "rolloff"), params))
    for k, v in params.items():
        if k not in ("zeros", "beta", "rolloff"):
            raise BPError("resample_params: unknown field %s" % k)
        setattr(rs, k, int(v) if k == "zeros" else float(v))
    return rs


def resample_ratio(rate_in, rate_out):
    """bp_resample_ratio: (p, q) with rate_out / rate_in = p / q in lowest terms, max(p, q) <= 1024; host only."""
    lib = load_library()
    p, q = C.c_int(), C.c_int()
    rc = lib.bp_resample_ratio(int(rate_in), int(rate_out), C.byref(p), C.byref(q))
    if rc != 0:
        _raise(lib, rc)
    return int(p.value), int(q.value)


def resample_len(n, p, q):
    """bp_resample_len: ceil(n p / q), the samples a sentence of n samples becomes; host only."""
    lib = load_library()
    out = C.c_int64()
    rc = lib.bp_resample_len(int(n), int(p), int(q), C.byref(out))
    if rc != 0:
        _raise(lib, rc)
    return int(out.value)


def resample_taps(p, q, params=None):
    """bp_resample_taps: the 2 zeros max(p, q) + 1 float32 taps of the conversion by p / q; host only."""
    lib = load_library()
    rs = resample_params(params)
    zeros = 16 if rs is None else int(rs.zeros)
    h = np.empty(max(2 * max(zeros, 0) * max(int(p), int(q), 0) + 1, 1), np.float32)
    rc = lib.bp_resample_taps(int(p), int(q), None if rs is None else C.byref(rs), _fp(h), h.size)
    if rc != 0:
        _raise(lib, rc)
    return h


def resample_waves(device, rate_in, rate_out, sentences, params=None):
    """bp_resample_waves: every sentence (1-D arrays) converted from rate_in to rate_out, a list of float32 arrays of
    resample_len samples each (no handle).  Defined to the bit in include/bp_c_api.h."""
    lib = load_library()
    rs = resample_params(params)
    p, q = resample_ratio(rate_in, rate_out)
    arrs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in sentences]
    lens = np.array([a.size for a in arrs], np.int32)
    pcm = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros(0, np.float32))
    n_out = (lens.astype(np.int64) * p + q - 1) // q
    out = np.empty(max(int(n_out.sum()), 1), np.float32)
    rc = lib.bp_resample_waves(int(device), int(rate_in), int(rate_out), None if rs is None else C.byref(rs), len(arrs),
                               lens.ctypes.data_as(C.POINTER(C.c_int)), _fp(pcm), _fp(out))
    if rc != 0:
        _raise(lib, rc)
    return np.split(out[:int(n_out.sum())], np.cumsum(n_out)[:-1])


def reverb_waves(device, sents, sent_rir, rirs, early_taps=0, early=True):
    """bp_reverb_waves: (rev, early) lists of the reverberant sentences and their direct-plus-early parts (None for early=False):
    sentence k convolved with rirs[sent_rir[k]], aligned to the direct path (include/bp_c_api.h).  No handle."""
    lib = load_library()
    ss = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in sents]
    hs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1) for x in rirs]
    slen = np.array([x.size for x in ss], np.int32)
    hlen = np.array([x.size for x in hs], np.int32)
    sr = np.ascontiguousarray(sent_rir, dtype=np.int32).reshape(-1)
    if sr.size != len(ss):
        raise BPError("reverb_waves: %d sentences but %d response indices" % (len(ss), sr.size))
    spcm = np.ascontiguousarray(np.concatenate(ss) if ss else np.zeros(0, np.float32))
    hpcm = np.ascontiguousarray(np.concatenate(hs) if hs else np.zeros(0, np.float32))
    n = int(slen.sum())
    rev = np.empty(max(n, 1), np.float32)
    ear = np.empty(max(n, 1), np.float32) if early else None
    ip = C.POINTER(C.c_int)
    rc = lib.bp_reverb_waves(int(device), len(ss), slen.ctypes.data_as(ip), _fp(spcm), sr.ctypes.data_as(ip), len(hs),
                             hlen.ctypes.data_as(ip), _fp(hpcm), int(early_taps), _fp(rev), _fp(ear) if early else None)
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    cut = np.cumsum(slen)[:-1]
    return np.split(rev[:n], cut), (np.split(ear[:n], cut) if early else None)


def rir_delay(h):
    """bp_mix_rir_delay: the first index at which |h[j]| is largest; host only."""
    lib = load_library()
    h = np.ascontiguousarray(h, dtype=np.float32).reshape(-1)
    d = C.c_int()
    rc = lib.bp_mix_rir_delay(_fp(h) if h.size else None, h.size, C.byref(d))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return int(d.value)


def mix_reverb_pairs(seed, n_clean, n_rir):
    """bp_mix_reverb_pairs: the response of every clean sentence (int32 [n_clean]), keyed by the seed; host only."""
    lib = load_library()
    out = np.zeros(max(int(n_clean), 1), np.int32)
    rc = lib.bp_mix_reverb_pairs(int(seed), int(n_clean), int(n_rir), out.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return out[:int(n_clean)]


def _rooms(rooms):
    r = np.ascontiguousarray(rooms, dtype=RIR_ROOM_DTYPE).reshape(-1)
    return r


def rir_window_default(sample_rate):
    """the delay window rir_image uses when none is given: 2 round(0.004 fs) taps (8 ms; halves round up)"""
    return 2 * int(np.floor(0.004 * int(sample_rate) + 0.5))


def rir_image(device, sample_rate, rooms, rir_len, window_taps=None):
    """bp_rir_image: a list of float32 arrays, response k of rir_len[k] taps for rooms[k] (RIR_ROOM_DTYPE) by the image method
    (include/bp_c_api.h); the list is what BP_GPU.set_mix_reverb takes.  No handle."""
    lib = load_library()
    r = _rooms(rooms)
    n = np.ascontiguousarray(rir_len, dtype=np.int32).reshape(-1)
    if n.size != r.size:
        raise BPError("rir_image: %d rooms but %d lengths" % (r.size, n.size))
    tw = rir_window_default(sample_rate) if window_taps is None else int(window_taps)
    out = np.zeros(max(int(np.clip(n, 0, MIX_RIR_MAX_TAPS).sum()), 1), np.float32)
    rc = lib.bp_rir_image(int(device), int(sample_rate), tw, int(r.size), r.ctypes.data_as(C.c_void_p) if r.size else None,
                          n.ctypes.data_as(C.POINTER(C.c_int)) if n.size else None, _fp(out))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return np.split(out[:int(n.sum())], np.cumsum(n)[:-1])


def rir_orders(room, sample_rate, n_taps, window_taps=None):
    """bp_rir_orders: ((N_0, N_1, N_2), images of the box) of one room; host only."""
    lib = load_library()
    r = _rooms(room)
    tw = rir_window_default(sample_rate) if window_taps is None else int(window_taps)
    order = np.zeros(3, np.int32)
    n = C.c_int64()
    rc = lib.bp_rir_orders(r.ctypes.data_as(C.c_void_p), int(sample_rate), int(n_taps), tw, order.ctypes.data_as(C.POINTER(C.c_int)),
                           C.byref(n))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return tuple(int(x) for x in order), int(n.value)


def rir_beta(L, t60):
    """bp_rir_beta: the six reflection coefficients (float64 [6]) Eyring's formula gives a box L for a NOMINAL t60; host only."""
    lib = load_library()
    Ld = np.ascontiguousarray(L, dtype=np.float64).reshape(-1)
    if Ld.size != 3:
        raise BPError("rir_beta: L needs 3 numbers")
    beta = np.zeros(6, np.float64)
    dp = C.POINTER(C.c_double)
    rc = lib.bp_rir_beta(Ld.ctypes.data_as(dp), float(t60), beta.ctypes.data_as(dp))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return beta


def rir_rooms(seed, n, **ranges):
    """bp_rir_rooms: n rooms (RIR_ROOM_DTYPE) drawn from the seed; ranges: L_lo, L_hi (3 numbers each), t60 and dist (lo, hi),
    margin -- RIR_RANGE_DEFAULTS where not given; host only."""
    lib = load_library()
    unknown = set(ranges) - set(RIR_RANGE_DEFAULTS)
    if unknown:
        raise BPError("rir_rooms: unknown range %s" % ", ".join(sorted(unknown)))
    g = dict(RIR_RANGE_DEFAULTS, **ranges)
    rg = BPRirRange()
    rg.L_lo[:] = [float(x) for x in g["L_lo"]]
    rg.L_hi[:] = [float(x) for x in g["L_hi"]]
    rg.t60_lo, rg.t60_hi = (float(x) for x in g["t60"])
    rg.dist_lo, rg.dist_hi = (float(x) for x in g["dist"])
    rg.margin = float(g["margin"])
    out = np.zeros(max(int(n), 1), RIR_ROOM_DTYPE)
    rc = lib.bp_rir_rooms(int(seed), int(n), C.byref(rg), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return out[:int(n)]


def mix_plan(seed, n_clean, per_clean, noise_lens, snr_list):
    """bp_mix_plan: the shuffled mixture list (MIXTURE_DTYPE [n_clean * per_clean]); host only."""
    lib = load_library()
    nl = np.ascontiguousarray(noise_lens, dtype=np.int64)
    snr = np.ascontiguousarray(snr_list, dtype=np.float32)
    out = np.zeros(max(int(n_clean) * int(per_clean), 1), MIXTURE_DTYPE)
    rc = lib.bp_mix_plan(int(seed), int(n_clean), int(per_clean), nl.size, nl.ctypes.data_as(C.POINTER(C.c_int64)), snr.size,
                         _fp(snr), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return out[:int(n_clean) * int(per_clean)]


def mix_shuffle(seed, stream, n):
    """bp_mix_shuffle: a permutation of range(n) (int32), keyed by (seed, stream); host only."""
    lib = load_library()
    out = np.zeros(max(int(n), 1), np.int32)
    rc = lib.bp_mix_shuffle(int(seed), int(stream), int(n), out.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))
    return out[:int(n)]


# ------------------------------------------------------------------ pre-training: stacked RBMs, CD-1 (bp_rbm_*)
RBM_HYPER_FIELDS = [f[0] for f in BPRbmHyper._fields_]


def rbm_defaults(layer):
    """bp_rbm_defaults: the hyper-parameters a new stack holds for RBM `layer`, as a dict."""
    lib = load_library()
    h = BPRbmHyper()
    rc = lib.bp_rbm_defaults(int(layer), C.byref(h))
    if rc != 0:
        _raise(lib, rc)
    return {k: getattr(h, k) for k in RBM_HYPER_FIELDS}


class RBMStack(object):
    """A stack of RBMs on the device (bp_rbm, include/bp_c_api.h); made by rbm_open."""

    def __init__(self, lib, s, layersizes, bunchsize):
        self._lib, self._s = lib, s
        self.layersizes, self.bunchsize = list(layersizes), int(bunchsize)
        self._hyper = {l: rbm_defaults(l) for l in range(1, len(self.layersizes))}

    def _check(self, rc):
        if rc != 0:
            _raise(self._lib, rc)

    def _rows(self, rows, n=None):
        a = np.ascontiguousarray(rows, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.layersizes[0] or (n is not None and a.shape[0] != n):
            raise BPError("rows must be [%s][%d]" % ("n" if n is None else n, self.layersizes[0]))
        return a

    def _layer(self, layer):
        if not 1 <= int(layer) < len(self.layersizes):
            raise BPError("layer must lie in [1, %d]" % (len(self.layersizes) - 1))
        return int(layer)

    def hyper(self, layer):
        return dict(self._hyper[self._layer(layer)])

    def set_hyper(self, layer, **fields):
        """bp_rbm_set_hyper: the named fields (lrate, momentum, weightcost, visible, sample) change, the others stay."""
        layer = self._layer(layer)
        bad = sorted(set(fields) - set(RBM_HYPER_FIELDS))
        if bad:
            raise BPError("unknown hyper-parameter: %s" % ", ".join(bad))
        new = dict(self._hyper[layer], **fields)
        h = BPRbmHyper(float(new["lrate"]), float(new["momentum"]), float(new["weightcost"]), int(new["visible"]), int(new["sample"]))
        self._check(self._lib.bp_rbm_set_hyper(self._s, layer, C.byref(h)))
        self._hyper[layer] = new

    def train(self, layer, rows):
        """bp_rbm_train_chunk: one CD-1 step per full bunch of rows; the sum of the bunches' reconstruction errors."""
        a = self._rows(rows)
        e = C.c_double(0.0)
        self._check(self._lib.bp_rbm_train_chunk(self._s, int(layer), a.shape[0], _fp(a), C.byref(e)))
        return e.value

    def up(self, layer, rows):
        """bp_rbm_up: the mean-field output of RBM `layer`, [n][layersizes[layer]]."""
        layer = self._layer(layer)
        a = self._rows(rows)
        out = np.empty((a.shape[0], self.layersizes[layer]), np.float32)
        self._check(self._lib.bp_rbm_up(self._s, layer, a.shape[0], _fp(a), _fp(out)))
        return out

    def step(self, layer, rows, apply=False):
        """bp_rbm_step on one bunch: every array of the trace (v0 p0 s0 v1 p1 gw gc ga) and recon, as a dict."""
        layer = self._layer(layer)
        a = self._rows(rows, self.bunchsize)
        V, H, B = self.layersizes[layer - 1], self.layersizes[layer], self.bunchsize
        out = dict(v0=np.empty((B, V), np.float32), p0=np.empty((B, H), np.float32), s0=np.empty((B, H), np.float32),
                   v1=np.empty((B, V), np.float32), p1=np.empty((B, H), np.float32), gw=np.empty((V, H), np.float32),
                   gc=np.empty(H, np.float32), ga=np.empty(V, np.float32))
        recon = C.c_double(0.0)
        tr = BPRbmTrace(*[_fp(out[k]) for k in ("v0", "p0", "s0", "v1", "p1", "gw", "gc", "ga")], C.pointer(recon))
        self._check(self._lib.bp_rbm_step(self._s, layer, _fp(a), 1 if apply else 0, C.byref(tr)))
        out["recon"] = recon.value
        return out

    def steps(self, layer):
        n = C.c_uint(0)
        self._check(self._lib.bp_rbm_steps(self._s, int(layer), C.byref(n)))
        return int(n.value)

    def get(self):
        """bp_rbm_get: (weights, hbias, vbias), lists indexed 1 .. numlayers-1 (entry 0 is None)."""
        L = len(self.layersizes)
        w, c, a = [None] * L, [None] * L, [None] * L
        for l in range(1, L):
            w[l] = np.empty((self.layersizes[l - 1], self.layersizes[l]), np.float32)
            c[l] = np.empty(self.layersizes[l], np.float32)
            a[l] = np.empty(self.layersizes[l - 1], np.float32)
        self._check(self._lib.bp_rbm_get(self._s, _ptrs(w), _ptrs(c), _ptrs(a)))
        return w, c, a

    def close(self):
        if self._s is not None:
            self._lib.bp_rbm_destroy(self._s)
            self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rbm_open(device, layersizes, bunchsize, weights, hbias, vbias=None, seed=0, max_chunk_frames=0):
    """bp_rbm_create: weights / hbias / vbias are lists indexed 1 .. len(layersizes)-1 (vbias None or entries None: zeros)."""
    lib = load_library()
    ls = [int(x) for x in layersizes]
    cfg = BPRbmConfig()
    cfg.device, cfg.numlayers, cfg.bunchsize = int(device), len(ls), int(bunchsize)
    for i, s in enumerate(ls[:MAXLAYER]):
        cfg.layersizes[i] = s
    cfg.max_chunk_frames, cfg.seed = int(max_chunk_frames), int(seed)

    def flat(arrs, sizes, name):
        out = [None] * MAXLAYER
        for l in range(1, min(len(ls), MAXLAYER)):
            if arrs is None or l >= len(arrs) or arrs[l] is None:
                continue
            out[l] = np.ascontiguousarray(arrs[l], dtype=np.float32).reshape(-1)
            if out[l].size != sizes(l):
                raise BPError("%s[%d] has the wrong size" % (name, l))
        return out
    w = flat(weights, lambda l: ls[l - 1] * ls[l], "weights")
    c = flat(hbias, lambda l: ls[l], "hbias")
    a = flat(vbias, lambda l: ls[l - 1], "vbias")
    s = C.c_void_p()
    rc = lib.bp_rbm_create(C.byref(cfg), _ptrs(w), _ptrs(c), _ptrs(a) if vbias is not None else None, C.byref(s))
    if rc != 0:
        _raise(lib, rc)
    return RBMStack(lib, s, ls, bunchsize)


def device_count():
    n = C.c_int()
    lib = load_library()
    if lib.bp_device_count(C.byref(n)) != 0:
        raise BPError(lib.bp_last_error().decode())
    return int(n.value)


def device_pci_bus_id(device):
    lib = load_library()
    buf = C.create_string_buffer(32)
    if lib.bp_device_pci_bus_id(int(device), buf, 32) != 0:
        raise BPError(lib.bp_last_error().decode())
    return buf.value.decode()


class Rendezvous(object):
    """bp_rdv_* (include/bp_c_api.h): the host-only rendezvous of the data-parallel ranks; works without a GPU."""

    def __init__(self, key, world, rank, timeout_s=30.0):
        self._lib = load_library()
        self.world, self.rank = int(world), int(rank)
        self._r = C.c_void_p()
        if self._lib.bp_rdv_open(str(key).encode(), self.world, self.rank, float(timeout_s), C.byref(self._r)) != 0:
            self._r = None
            raise BPError(self._lib.bp_last_error().decode())

    def barrier(self):
        if self._lib.bp_rdv_barrier(self._r) != 0:
            raise BPError(self._lib.bp_last_error().decode())

    def allgather_f64(self, value):
        mine = (C.c_double * 1)(float(value))
        out = (C.c_double * self.world)()
        if self._lib.bp_rdv_allgather(self._r, mine, 8, out) != 0:
            raise BPError(self._lib.bp_last_error().decode())
        return [float(v) for v in out]

    def close(self):
        if self._r is not None:
            self._lib.bp_rdv_close(self._r)
            self._r = None
