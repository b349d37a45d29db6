"""MI355X-native replacement of the reference's frame-wise DNN trainer hot path
(`BP_GPU` in yongxuUSTC/DNN-for-speech-enhancement).  The product is the gfx950 HIP library
`libbp_hip.so` behind the C ABI in include/bp_c_api.h; this package is its Python host mirror.
(The directory name contains '-', import it through `dnnse_amd.py` at the repo root.)"""
from .bp_gpu import (BP_GPU, BPError, BPConfig, load_library, LIB_PATH, ABI_SYMBOLS, MAXLAYER, MAXCACHEFRAME,  # noqa: F401
                     Rendezvous, device_count, device_pci_bus_id, wave_lps, WAVE_LPS, WAVE_MASK, FORWARD_DEFAULT, FORWARD_ROWINV,
                     BPWaveChunk, BPMixCorpus, MIXTURE_DTYPE, MIX_TARGETS, MIX_LPS, MIX_IRM, MIX_IBM, MIX_LPS_IRM,
                     MIX_LPS_IBM, mix_plan, mix_shuffle, BPMixReverb, REVERB_TARGETS, REVERB_TARGET_REVERBERANT,
                     REVERB_TARGET_EARLY, MIX_RIR_MAX_TAPS, reverb_waves, rir_delay, mix_reverb_pairs, score_waves, SCORE_SSNR, SCORE_LSD, SCORE_STOI,
                     SCORE_ESTOI, SCORE_SISDR,
                     BPStreamConfig, Stream, stream_counts, BPLogmmseParams, logmmse_params, logmmse_waves,
                     LogmmseStream, logmmse_stream_open, logmmse_stream_counts, BPNoiseParams, noise_params, NOISE_VAD, NOISE_SPP,
                     NAT_STATIC, NAT_DYNAMIC, NAT_MODES,
                     rir_image, rir_rooms, rir_beta, rir_orders, rir_window_default, BPRirRange, RIR_ROOM_DTYPE, RIR_RANGE_DEFAULTS,
                     RIR_MAX_IMAGES,
                     BPResampleParams, resample_waves, resample_ratio, resample_len, resample_taps, resample_params,
                     BPMelParams, mel_params, mel_filters, mel_dct, wave_mfcc,
                     BPPostParams, post_params, post_rows, gv_factors, GV_RAW, GV_POST, GV_STAGES, GV_INDEP, GV_DEP, GV_MODES,
                     BPRbmConfig, BPRbmHyper, BPRbmTrace, RBMStack, rbm_open, rbm_defaults)
from .weights_init import glorot_net  # noqa: F401
