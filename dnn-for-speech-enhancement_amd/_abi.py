"""The C ABI of include/bp_c_api.h as ctypes sees it, in one place: the constants that mirror the header's enums, the Structure
mirrors and numpy record dtypes of its structs, the signature of every entry point (ABI), and load_library, which applies the
table once when the library is loaded.  tests/test_abi.py holds all of it to the header.  Below the table: the few idioms every
wrapper module shares (status to BPError, parameter structs, packed sentences, array pointers, close-on-exit)."""
import ctypes as C
import os

import numpy as np

__all__ = [
    "MAXLAYER", "MAXCACHEFRAME", "LIB_PATH", "ABI_SYMBOLS", "BPError", "load_library",
    "WAVE_LPS", "WAVE_MASK", "FORWARD_DEFAULT", "FORWARD_ROWINV", "NAT_STATIC", "NAT_DYNAMIC", "NAT_MODES",
    "GV_RAW", "GV_POST", "GV_STAGES", "GV_INDEP", "GV_DEP", "GV_MODES",
    "MIX_LPS", "MIX_IRM", "MIX_IBM", "MIX_LPS_IRM", "MIX_LPS_IBM", "MIX_TARGETS", "MIXTURE_DTYPE",
    "SCORE_SSNR", "SCORE_LSD", "SCORE_STOI", "SCORE_ESTOI", "SCORE_SISDR", "SCORE_LLR", "SCORE_CD", "SCORE_FULL_N",
    "SCORE_FWSSNR", "SCORE_WSS", "SCORE_ALL_N",
    "REVERB_TARGET_REVERBERANT", "REVERB_TARGET_EARLY", "REVERB_TARGETS", "MIX_RIR_MAX_TAPS",
    "RIR_MAX_IMAGES", "RIR_ROOM_DTYPE", "RIR_RANGE_DEFAULTS", "NOISE_VAD", "NOISE_SPP", "PROF_KINDS",
    "BPConfig", "BPWindowChunk", "BPWaveChunk", "BPMixCorpus", "BPMixReverb", "BPRirRange", "BPStreamConfig",
    "BPLogmmseParams", "BPNoiseParams", "BPResampleParams", "BPMelParams", "BPPostParams",
    "BPRbmConfig", "BPRbmHyper", "BPRbmTrace",
]

MAXLAYER = 10          # BP_GPU.h:13
MAXCACHEFRAME = 200000  # BP_GPU.h:14

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libbp_hip.so")

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
SCORE_LLR, SCORE_CD, SCORE_FULL_N = 5, 6, 7   # the two behind those (extended="full") and the width of such a row
SCORE_FWSSNR, SCORE_WSS, SCORE_ALL_N = 7, 8, 9   # fwSegSNR and WSS behind those (extended="all") and the width of such a row
REVERB_TARGET_REVERBERANT, REVERB_TARGET_EARLY = 0, 1   # bp_mix_reverb.target
REVERB_TARGETS = {"reverberant": REVERB_TARGET_REVERBERANT, "early": REVERB_TARGET_EARLY}
MIX_RIR_MAX_TAPS = 65536
RIR_MAX_IMAGES = 1 << 26
NOISE_VAD, NOISE_SPP = 0, 1              # bp_noise_params.mode
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


I, F, D, I64, U64, U32, SZ = C.c_int, C.c_float, C.c_double, C.c_int64, C.c_uint64, C.c_uint32, C.c_size_t
P = C.POINTER
ip, fp, dp, lp, fpp = P(I), P(F), P(D), P(I64), P(P(F))


class BPWindowChunk(C.Structure):
    """bp_window_chunk (include/bp_c_api.h): raw frames + index tables, stacked on the device."""
    _fields_ = [
        ("n_samples", I), ("n_frames", I), ("fea_dim", I), ("context", I), ("n_nat", I),
        ("fea", fp), ("targ_frames", fp), ("nat", fp),
        ("win_start", ip), ("targ_frame", ip), ("nat_row", ip),
    ]


class BPWaveChunk(C.Structure):
    """bp_wave_chunk (include/bp_c_api.h): noisy sentences for bp_enhance_waves."""
    _fields_ = [
        ("n_sent", I), ("sent_len", ip), ("pcm", fp),
        ("context", I), ("targ_offset", I),
        ("mean", fp), ("inv_std", fp),
        ("target", I), ("out_col", I),
    ]


class BPMixCorpus(C.Structure):
    """bp_mix_corpus (include/bp_c_api.h): clean and noise recordings, resident on the handle."""
    _fields_ = [
        ("fea_dim", I), ("context", I), ("targ_offset", I), ("target", I), ("lc_db", F),
        ("mean", fp), ("inv_std", fp),
        ("n_clean", I), ("clean_len", lp), ("clean_pcm", fp),
        ("n_noise", I), ("noise_len", lp), ("noise_pcm", fp),
    ]


class BPMixReverb(C.Structure):
    """bp_mix_reverb (include/bp_c_api.h): impulse responses and the {clean, response} pairs that become derived entries."""
    _fields_ = [
        ("n_rir", I), ("rir_len", ip), ("rir_pcm", fp),
        ("n_pair", I), ("pair_clean", ip), ("pair_rir", ip),
        ("target", I), ("early_taps", I),
    ]


class BPRirRange(C.Structure):
    """bp_rir_range (include/bp_c_api.h): the ranges bp_rir_rooms draws rooms from."""
    _fields_ = [
        ("L_lo", D * 3), ("L_hi", D * 3), ("t60_lo", D), ("t60_hi", D),
        ("margin", D), ("dist_lo", D), ("dist_hi", D),
    ]


class BPStreamConfig(C.Structure):
    """bp_stream_config (include/bp_c_api.h): a streaming session of n_chan channels."""
    _fields_ = [
        ("fea_dim", I), ("context", I), ("targ_offset", I),
        ("mean", fp), ("inv_std", fp),
        ("target", I), ("out_col", I), ("n_chan", I), ("max_push_samples", I),
    ]


class BPLogmmseParams(C.Structure):
    """bp_logmmse_params (include/bp_c_api.h): the log-MMSE baseline's parameters."""
    _fields_ = [
        ("alpha", D), ("mu", D), ("eta", D), ("xi_min_db", D), ("gamma_max", D),
        ("init_frames", I),
    ]


class BPNoiseParams(C.Structure):
    """bp_noise_params (include/bp_c_api.h): the noise update of the log-MMSE baseline."""
    _fields_ = [
        ("mode", I), ("xi_h1_db", D), ("q", D), ("a_pow", D), ("a_spp", D),
        ("p_lo", D), ("p_cap", D),
    ]


class BPResampleParams(C.Structure):
    """bp_resample_params (include/bp_c_api.h): the windowed-sinc filter of the sample-rate converter."""
    _fields_ = [("zeros", I), ("beta", D), ("rolloff", D)]


class BPMelParams(C.Structure):
    """bp_mel_params (include/bp_c_api.h): the MFCC auxiliary target.  mean / scale point into arrays the owner keeps alive
    (mel_params stores them on the object)."""
    _fields_ = [
        ("sample_rate", I), ("n_mel", I), ("n_ceps", I), ("first_coef", I),
        ("f_lo", F), ("f_hi", F), ("lifter", F),
        ("mean", fp), ("scale", fp),
    ]


class BPPostParams(C.Structure):
    """bp_post_params (include/bp_c_api.h): post-processing of the LPS estimate.  gv_center / gv_scale point into arrays the owner
    keeps alive (post_params stores them on the object)."""
    _fields_ = [
        ("gv", I), ("gv_center", fp), ("gv_scale", fp),
        ("mask_col", I), ("mask_lo", F), ("mask_hi", F), ("mask_weight", F),
    ]


class BPRbmConfig(C.Structure):
    """bp_rbm_config (include/bp_c_api.h): a stack of RBMs."""
    _fields_ = [
        ("device", I), ("numlayers", I), ("layersizes", I * MAXLAYER),
        ("bunchsize", I), ("max_chunk_frames", I), ("seed", U64),
    ]


class BPRbmHyper(C.Structure):
    """bp_rbm_hyper (include/bp_c_api.h): the hyper-parameters of one RBM's CD-1 step."""
    _fields_ = [("lrate", F), ("momentum", F), ("weightcost", F), ("visible", I), ("sample", I)]


class BPRbmTrace(C.Structure):
    """bp_rbm_trace (include/bp_c_api.h): what bp_rbm_step hands back; any pointer may be NULL."""
    _fields_ = [
        ("v0", fp), ("p0", fp), ("s0", fp), ("v1", fp),
        ("p1", fp), ("gw", fp), ("gc", fp), ("ga", fp),
        ("recon", dp),
    ]


class BPConfig(C.Structure):
    _fields_ = [
        ("gpu_used", I), ("numlayers", I), ("layersizes", I * MAXLAYER),
        ("bunchsize", I), ("lrate", F), ("momentum", F), ("weightcost", F),
        ("dropoutflag", I), ("visible_omit", F), ("hid_omit", F),
        ("activation", I), ("momentum_rule", I), ("seed", U64), ("device", I),
        ("global_bunchsize", I), ("rank_frame_offset", I), ("max_chunk_frames", I),
        ("compute_dtype", I),
    ]


# ---- what stands for each `typedef struct` of the header
STRUCTS = {       # a Structure the wrappers build: a pointer to it is POINTER(<mirror>)
    "bp_config": BPConfig, "bp_window_chunk": BPWindowChunk, "bp_wave_chunk": BPWaveChunk, "bp_mix_corpus": BPMixCorpus,
    "bp_mix_reverb": BPMixReverb, "bp_rir_range": BPRirRange, "bp_stream_config": BPStreamConfig,
    "bp_logmmse_params": BPLogmmseParams, "bp_noise_params": BPNoiseParams, "bp_resample_params": BPResampleParams,
    "bp_mel_params": BPMelParams, "bp_post_params": BPPostParams, "bp_rbm_config": BPRbmConfig, "bp_rbm_hyper": BPRbmHyper,
    "bp_rbm_trace": BPRbmTrace,
}
DTYPES = {        # arrays of it live in numpy: a pointer to it is the c_void_p of the array's block
    "bp_mixture": MIXTURE_DTYPE, "bp_rir_room": RIR_ROOM_DTYPE,
}
NOT_MIRRORED = {  # never built in Python, with the reason: a pointer to it is a c_void_p
    "bp_handle": "opaque handle (bp_create)", "bp_stream": "opaque handle (bp_stream_open)",
    "bp_lmstream": "opaque handle (bp_lmstream_open)", "bp_rdv": "opaque handle (bp_rdv_open)",
    "bp_rbm": "opaque handle (bp_rbm_create)",
}

# ---- the signature of every entry point: {symbol: argtypes}; every one returns int (a bp_status) but those of ABI_RESTYPES
H = V = C.c_void_p            # H: an opaque handle; V: void *, or the block of a DTYPES array
HP = P(C.c_void_p)            # where a call returns a handle
LM, NZ, MEL, POST, RS = P(BPLogmmseParams), P(BPNoiseParams), P(BPMelParams), P(BPPostParams), P(BPResampleParams)
WIN = P(BPWindowChunk)
_PUSH = [H, ip, fp, P(C.c_ubyte), ip, fp, SZ]
ABI_RESTYPES = {"bp_last_error": C.c_char_p, "bp_build_target": C.c_char_p}
ABI = {
    "bp_last_error": [], "bp_abi_version": [], "bp_build_target": [], "bp_create": [P(BPConfig), fpp, fpp, HP], "bp_destroy": [H],
    "bp_train_chunk": [H, I, fp, fp], "bp_cv_chunk": [H, I, fp, fp, fp], "bp_forward": [H, I, fp, fp],
    "bp_get_weights": [H, fpp, fpp], "bp_get_deltas": [H, fpp, fpp], "bp_upload_chunk": [H, I, fp, fp],
    "bp_fill_chunk_synthetic": [H, I, U64], "bp_train_resident": [H, I, I], "bp_sync": [H], "bp_grads_resident": [H, I],
    "bp_grad_layout": [H, I, P(SZ), P(SZ)], "bp_grad_floats": [H, P(SZ)], "bp_read_grads": [H, fp, SZ],
    "bp_read_layer_output": [H, I, fp, SZ], "bp_last_train_ms": [H, fp, ip], "bp_time_kernel": [H, I, I, fp],
    "bp_upload_chunk_windows": [H, WIN], "bp_train_chunk_windows": [H, WIN], "bp_cv_chunk_windows": [H, WIN, fp],
    "bp_set_hyper": [H, F, F, F, I, F, F], "bp_set_output": [H, I, I, I], "bp_set_forward": [H, I],
    "bp_dp_attach": [H, I, I, C.c_char_p], "bp_dp_attach_ex": [H, I, I, C.c_char_p, I], "bp_dp_detach": [H],
    "bp_dp_info": [H, ip, ip, P(U32)], "bp_dp_peer_info": [H, I, ip, C.c_char_p, I, ip, ip], "bp_dp_handoff": [H, ip],
    "bp_dp_barrier": [H], "bp_dp_allgather": [H, V, SZ, V], "bp_rdv_open": [C.c_char_p, I, I, D, HP], "bp_rdv_barrier": [H],
    "bp_rdv_allgather": [H, V, SZ, V], "bp_rdv_close": [H], "bp_device_pci_bus_id": [I, C.c_char_p, I], "bp_host_register": [V, SZ],
    "bp_host_unregister": [V], "bp_profile_step": [H, I, I, fp, ip], "bp_measure_peaks": [H, fp, fp], "bp_device_count": [ip],
    "bp_train_resident_masked": [H, I, I, P(P(C.c_uint8))], "bp_forward_windows": [H, WIN, fp],
    "bp_enhance_waves": [H, I, P(BPWaveChunk), fp, fp], "bp_wave_lps": [I, I, I, ip, fp, fp],
    "bp_set_mix_corpus": [H, P(BPMixCorpus)], "bp_train_mix": [H, I, V, ip], "bp_cv_mix": [H, I, V, fp],
    "bp_mix_features": [H, I, V, fp, fp, fp, fp, fp], "bp_mix_plan": [U64, I, I, I, lp, I, fp, V],
    "bp_mix_shuffle": [U64, U32, I, ip], "bp_set_mix_reverb": [H, P(BPMixReverb)],
    "bp_reverb_waves": [I, I, ip, fp, ip, I, ip, fp, I, fp, fp], "bp_mix_rir_delay": [fp, I, ip],
    "bp_mix_reverb_pairs": [U64, I, I, ip], "bp_rir_image": [I, I, I, I, V, ip, fp], "bp_rir_orders": [V, I, I, I, ip, lp],
    "bp_rir_beta": [dp, D, dp], "bp_rir_rooms": [U64, I, P(BPRirRange), V], "bp_score_waves": [I, I, I, I, ip, fp, fp, fp],
    "bp_eval_mix": [H, I, V, I, I, I, fp, fp, fp], "bp_score_waves_ext": [I, I, I, I, ip, fp, fp, I, fp],
    "bp_eval_mix_ext": [H, I, V, I, I, I, I, fp, fp, fp], "bp_eval_mix_logmmse_ext": [H, LM, I, V, I, I, fp, fp, fp],
    "bp_stream_open": [H, P(BPStreamConfig), HP], "bp_stream_push": _PUSH, "bp_stream_close": [H],
    "bp_stream_counts": [I, I, I, I, I64, I, lp, lp, lp], "bp_stream_packed": [H], "bp_logmmse_defaults": [LM],
    "bp_logmmse_waves": [I, I, LM, I, ip, fp, fp, fp, fp], "bp_eval_mix_logmmse": [H, LM, I, V, I, fp, fp, fp],
    "bp_lmstream_open": [I, I, LM, I, I, HP], "bp_lmstream_push": _PUSH, "bp_lmstream_close": [H],
    "bp_lmstream_counts": [I, I, I64, I, lp, lp, lp], "bp_noise_defaults": [NZ],
    "bp_logmmse_waves_nt": [I, I, LM, NZ, I, ip, fp, fp, fp, fp, fp], "bp_eval_mix_logmmse_nt": [H, LM, NZ, I, V, I, I, fp, fp, fp],
    "bp_lmstream_open_nt": [I, I, LM, NZ, I, I, HP], "bp_set_nat": [H, I, NZ], "bp_resample_defaults": [RS],
    "bp_resample_ratio": [I, I, ip, ip], "bp_resample_len": [I64, I, I, lp], "bp_resample_taps": [I, I, RS, fp, I],
    "bp_resample_waves": [I, I, I, RS, I, ip, fp, fp], "bp_mel_defaults": [I, MEL], "bp_mel_filters": [I, MEL, fp, ip, ip],
    "bp_mel_dct": [MEL, fp], "bp_wave_mfcc": [I, I, MEL, I, ip, fp, fp, fp, fp], "bp_set_mix_aux": [H, MEL],
    "bp_post_defaults": [POST], "bp_set_post": [H, I, POST], "bp_post_rows": [I, I, I, fp, fp, fp, POST, fp],
    "bp_gv_mix": [H, I, V, I, I, dp, dp, dp, dp, lp], "bp_gv_factors": [I, I64, dp, dp, dp, dp, I, fp, fp],
    "bp_rbm_defaults": [I, P(BPRbmHyper)], "bp_rbm_create": [P(BPRbmConfig), fpp, fpp, fpp, HP], "bp_rbm_destroy": [H],
    "bp_rbm_set_hyper": [H, I, P(BPRbmHyper)], "bp_rbm_train_chunk": [H, I, I, fp, dp], "bp_rbm_up": [H, I, I, fp, fp],
    "bp_rbm_step": [H, I, fp, I, P(BPRbmTrace)], "bp_rbm_steps": [H, I, P(U32)], "bp_rbm_get": [H, fpp, fpp, fpp],
}
ABI_SYMBOLS = list(ABI)       # every symbol include/bp_c_api.h declares (in the order they were added)

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
    for name, argtypes in ABI.items():
        fn = getattr(lib, name)
        fn.restype = ABI_RESTYPES.get(name, C.c_int)
        fn.argtypes = list(argtypes) or None      # (a call without parameters stays undeclared, as ctypes made it)
    if path is None:
        _lib = lib
    return lib


# ------------------------------------------------------------------ the idioms the wrappers share
def check(lib, rc):
    """A status of the library to BPError: "<bp_last_error> (status <rc>)"."""
    if rc != 0:
        raise BPError("%s (status %d)" % (lib.bp_last_error().decode(), rc))


def score_columns(who, extended):
    """n_scores of an _ext call for a wrapper's extended=: False 3, True 5, "full" 7, "all" 9; anything else is a BPError of `who`."""
    if isinstance(extended, (bool, np.bool_)):
        return 5 if extended else 3
    if isinstance(extended, str) and extended == "full":
        return SCORE_FULL_N
    if isinstance(extended, str) and extended == "all":
        return SCORE_ALL_N
    raise BPError("%s: extended must be False, True or \"full\", or \"all\" for the nine columns, not %r" % (who, extended))


_PTR = {np.dtype(np.float32): fp, np.dtype(np.int32): ip, np.dtype(np.float64): dp, np.dtype(np.int64): lp,
        np.dtype(np.uint8): P(C.c_ubyte)}


def ptr(a):
    """The float* / int* / double* / int64_t* / unsigned char* of a contiguous array of that dtype; None (NULL) for None."""
    return None if a is None else a.ctypes.data_as(_PTR[a.dtype])


def ptrs(arrs):
    """float *[MAXLAYER] over per-layer arrays (NULL where None)."""
    out = (fp * MAXLAYER)()
    for i, a in enumerate(arrs):
        if a is not None:
            out[i] = a.ctypes.data_as(fp)
    return out


def flat32(x):
    return np.ascontiguousarray(x, dtype=np.float32).reshape(-1)


def pack(seqs, fea_dim=None, lens=np.int32):
    """Sequences back to back as the library takes them: (concatenated float32 samples, int32 lengths -- or of the dtype lens --
    and with a fea_dim the int64 frame count of every sentence, T = (n-1)/hop + 2, else None)."""
    arrs = [flat32(x) for x in seqs]
    lens = np.array([a.size for a in arrs], lens)
    pcm = np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros(0, np.float32)
    if fea_dim is None:
        return pcm, lens, None
    hop = max(fea_dim - 1, 1)
    return pcm, lens, np.where(lens > 0, (lens - 1) // hop + 2, 0).astype(np.int64)


def split(flat, counts):
    """The inverse of pack on an output buffer: one view per sequence, counts[k] rows each (lengths or frame counts)."""
    return np.split(flat[:int(counts.sum())], np.cumsum(counts)[:-1])


_CAST = {I: int, I64: int, U64: int, F: float, D: float}


def set_fields(p, who, fields, skip=()):
    """Assign the Structure p by field name, each value cast as the field's ctypes type asks; names in skip are the caller's
    (pointers, strings).  An unknown name: BPError "<who>: unknown field <name>"."""
    types = dict(p._fields_)
    for k, v in fields.items():
        if k not in types:
            raise BPError("%s: unknown field %s" % (who, k))
        if k not in skip:
            setattr(p, k, _CAST[types[k]](v))
    return p


def struct_params(cls, defaults, who, fields, *args, **kw):
    """A cls filled by the library's bp_<x>_defaults(*args, &p), then overridden by field name (set_fields)."""
    lib = load_library()
    p = cls()
    check(lib, getattr(lib, defaults)(*(args + (C.byref(p),))))
    return set_fields(p, who, fields, **kw)


class Closing(object):
    """close() at the end of a with block and when the object is collected."""

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
