"""The signal layer of include/bp_c_api.h that needs no handle: analysis (wave_lps, the MFCC target), post-processing rows, the
log-MMSE baseline and its stream, scores, resampling, reverberation and room simulation, mixture plans and shuffles."""
import ctypes as C

import numpy as np

from ._abi import (BPError, BPLogmmseParams, BPMelParams, BPNoiseParams, BPPostParams, BPResampleParams, BPRirRange, Closing,
                   GV_MODES, MIX_RIR_MAX_TAPS, MIXTURE_DTYPE, NOISE_SPP, NOISE_VAD, RIR_RANGE_DEFAULTS, RIR_ROOM_DTYPE, check,
                   flat32, load_library, pack, ptr, score_columns, set_fields, split, struct_params)

__all__ = [
    "wave_lps", "post_params", "post_rows", "gv_factors", "mel_params", "mel_filters", "mel_dct", "wave_mfcc",
    "logmmse_params", "noise_params", "logmmse_waves", "LogmmseStream", "logmmse_stream_open", "logmmse_stream_counts",
    "stream_counts", "score_waves", "resample_params", "resample_ratio", "resample_len", "resample_taps", "resample_waves",
    "reverb_waves", "rir_delay", "mix_reverb_pairs", "rir_window_default", "rir_image", "rir_orders", "rir_beta", "rir_rooms",
    "mix_plan", "mix_shuffle",
]


def stream_push(lib_call, handle, n_chan, blocks, end, out_cap):
    """One push of either kind of stream (bp_stream_push, bp_lmstream_push): (status, one float32 array per channel or None).
    out_cap: samples of the output buffer, or a function of the samples pushed that gives them."""
    pcm, n_in, _ = pack(np.zeros(0, np.float32) if b is None else b for b in blocks)
    e = None if end is None else np.ascontiguousarray([1 if v else 0 for v in end], dtype=np.uint8)
    if callable(out_cap):
        out_cap = out_cap(int(pcm.size))
    out = np.empty(max(int(out_cap), 1), np.float32)
    n_out = np.zeros(n_chan, np.int32)
    rc = lib_call(handle, ptr(n_in), ptr(pcm) if pcm.size else None, ptr(e), ptr(n_out), ptr(out), int(out_cap))
    return rc, None if rc != 0 else [a.copy() for a in split(out, n_out)]


def _counts3(fn, *args):
    """(frames_in, frames_out, samples_out) from the count call named fn (bp_stream_counts, bp_lmstream_counts); host only."""
    lib = load_library()
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib, getattr(lib, fn)(*(args + (C.byref(a), C.byref(b), C.byref(c)))))
    return int(a.value), int(b.value), int(c.value)


def stream_counts(fea_dim, context, targ_offset, nat, received, ended):
    """bp_stream_counts: (frames_in, frames_out, samples_out) of a channel after `received` samples of its sentence; host only."""
    return _counts3("bp_stream_counts", int(fea_dim), int(context), int(targ_offset), 1 if nat else 0, int(received),
                    1 if ended else 0)


def wave_lps(device, fea_dim, sentences):
    """bp_wave_lps: the log-power spectrum of every sentence, one [T_s][fea_dim] float32 array each (no handle)."""
    lib = load_library()
    pcm, lens, frames = pack(sentences, int(fea_dim))
    out = np.empty((max(int(frames.sum()), 1), int(fea_dim)), np.float32)
    check(lib, lib.bp_wave_lps(int(device), int(fea_dim), len(lens), ptr(lens), ptr(pcm), ptr(out)))
    return split(out, frames)


def post_params(gv_center=None, gv_scale=None, mask_col=-1, mask_lo=0.5, mask_hi=0.5, mask_weight=1.0):
    """A BPPostParams over bp_post_defaults: GV on when gv_center and gv_scale are given (both or neither)."""
    p = struct_params(BPPostParams, "bp_post_defaults", "post_params",
                      dict(mask_col=mask_col, mask_lo=mask_lo, mask_hi=mask_hi, mask_weight=mask_weight))
    if (gv_center is None) != (gv_scale is None):
        raise BPError("post_params: gv_center and gv_scale come together")
    if gv_center is not None:
        p._center, p._scale = flat32(gv_center), flat32(gv_scale)       # (the struct holds pointers into them)
        if p._center.size != p._scale.size:
            raise BPError("post_params: gv_center and gv_scale differ in length")
        p.gv, p.gv_center, p.gv_scale = 1, ptr(p._center), ptr(p._scale)
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
    check(lib, lib.bp_post_rows(int(device), est.shape[1], est.shape[0], ptr(est), ptr(m), ptr(y), C.byref(p), ptr(out)))
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
    check(lib, lib.bp_gv_factors(D, int(stats["frames"]), *[ptr(a) for a in s], GV_MODES[mode], ptr(center), ptr(scale)))
    return center[:D], scale[:D]


def mel_params(sample_rate, **fields):
    """A BPMelParams: bp_mel_defaults(sample_rate) -- 26 filters, 13 coefficients from c0, 0 .. sample_rate / 2, lifter 22, no mean
    or scale -- overridden by the fields given (n_mel, n_ceps, first_coef, f_lo, f_hi, lifter; mean, scale: n_ceps values each).  A
    weight alpha_r on coefficient r's squared error is scale_r * sqrt(alpha_r)."""
    if "sample_rate" in fields:
        raise BPError("mel_params: unknown field sample_rate")
    mp = struct_params(BPMelParams, "bp_mel_defaults", "mel_params", fields, int(sample_rate), skip=("mean", "scale"))
    for k in ("mean", "scale"):
        if fields.get(k) is not None:
            a = flat32(fields[k])
            if a.size != mp.n_ceps:
                raise BPError("mel_params: %s must hold n_ceps = %d values, not %d" % (k, mp.n_ceps, a.size))
            setattr(mp, "_keep_" + k, a)                    # (the struct holds a pointer into it)
            setattr(mp, k, ptr(a))
    return mp


def mel_filters(fea_dim, mel):
    """bp_mel_filters: (w [n_mel][fea_dim] float32, first_bin [n_mel], n_bins [n_mel]) -- the triangles and the bins with w > 0; host only."""
    lib = load_library()
    n = max(int(mel.n_mel), 0)
    w = np.zeros((n, max(int(fea_dim), 1)), np.float32)
    first, nb = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    check(lib, lib.bp_mel_filters(int(fea_dim), C.byref(mel), ptr(w) if w.size else None, ptr(first), ptr(nb)))
    return w, first[:n], nb[:n]


def mel_dct(mel):
    """bp_mel_dct: t [n_ceps][n_mel] float32, the liftered DCT-II rows first_coef .. first_coef + n_ceps - 1; host only."""
    lib = load_library()
    n, c = max(int(mel.n_mel), 0), max(int(mel.n_ceps), 0)
    t = np.zeros((c, n), np.float32)
    check(lib, lib.bp_mel_dct(C.byref(mel), ptr(t) if t.size else None))
    return t


def wave_mfcc(device, fea_dim, sentences, mel, return_logmel=False, return_power=False):
    """bp_wave_mfcc: the MFCC target rows of every sentence, one [T_s][n_ceps] float32 array each (mean and scale applied; no
    handle).  With return_logmel / return_power a dict of mfcc and logmel [T_s][n_mel] / power [T_s][fea_dim] lists."""
    lib = load_library()
    pcm, lens, frames = pack(sentences, int(fea_dim))
    T = max(int(frames.sum()), 1)
    n_mel, n_ceps = max(int(mel.n_mel), 1), max(int(mel.n_ceps), 1)
    cc = np.empty((T, n_ceps), np.float32)
    lm = np.empty((T, n_mel), np.float32) if return_logmel else None
    pw = np.empty((T, int(fea_dim)), np.float32) if return_power else None
    check(lib, lib.bp_wave_mfcc(int(device), int(fea_dim), C.byref(mel), len(lens), ptr(lens), ptr(pcm), ptr(pw), ptr(lm), ptr(cc)))
    out = {"mfcc": split(cc, frames)}
    if not return_logmel and not return_power:
        return out["mfcc"]
    if return_logmel:
        out["logmel"] = split(lm, frames)
    if return_power:
        out["power"] = split(pw, frames)
    return out


def logmmse_params(params=None):
    """None (the library's defaults), or a BPLogmmseParams: bp_logmmse_defaults overridden by the fields of a dict."""
    if params is None or isinstance(params, BPLogmmseParams):
        return params
    return struct_params(BPLogmmseParams, "bp_logmmse_defaults", "logmmse_params", dict(params))


def noise_params(noise=None):
    """A BPNoiseParams: bp_noise_defaults (the MMSE-SPP tracker) for None or "spp", the VAD-gated update for "vad", the defaults
    overridden by the fields of a dict (mode: 0 / 1 or "vad" / "spp"), or the BPNoiseParams given."""
    if isinstance(noise, BPNoiseParams):
        return noise
    modes = {"vad": NOISE_VAD, "spp": NOISE_SPP}
    noise = {} if noise is None else {"mode": noise} if isinstance(noise, str) else dict(noise)
    if isinstance(noise.get("mode"), str):
        if noise["mode"] not in modes:
            raise BPError("noise_params: unknown mode %s" % noise["mode"])
        noise["mode"] = modes[noise["mode"]]
    return struct_params(BPNoiseParams, "bp_noise_defaults", "noise_params", noise)


def _ref(p):
    """A parameter struct, or None for the library's defaults, as the pointer argument."""
    return None if p is None else C.byref(p)


def logmmse_waves(device, fea_dim, sentences, params=None, return_gain=False, return_vad=False, noise=None, return_noise=False):
    """bp_logmmse_waves: every sentence enhanced by the log-MMSE baseline (no handle, no net): a list of float32 arrays, or with
    return_gain / return_vad / return_noise a tuple (pcm, gain [T_s][fea_dim] per sentence, vad [T_s] per sentence, noise
    [T_s][fea_dim] per sentence; the ones not asked for omitted).  noise: None for the call as it always was, else "spp", "vad",
    a dict of bp_noise_params fields or a BPNoiseParams (noise_params): bp_logmmse_waves_nt.  return_noise needs the latter call
    and, with noise None, makes it in VAD mode: the same bits, and the lambda every frame's gamma used."""
    lib = load_library()
    pcm, lens, frames = pack(sentences, int(fea_dim))
    T = max(int(frames.sum()), 1)
    out = np.empty(max(pcm.size, 1), np.float32)
    gain = np.empty((T, int(fea_dim)), np.float32) if return_gain else None
    vad = np.empty(T, np.float32) if return_vad else None
    nse = np.empty((T, int(fea_dim)), np.float32) if return_noise else None
    lm = _ref(logmmse_params(params))
    if noise is None and not return_noise:
        rc = lib.bp_logmmse_waves(int(device), int(fea_dim), lm, len(lens), ptr(lens), ptr(pcm), ptr(out), ptr(gain), ptr(vad))
    else:
        nz = noise_params("vad" if noise is None else noise)
        rc = lib.bp_logmmse_waves_nt(int(device), int(fea_dim), lm, C.byref(nz), len(lens), ptr(lens), ptr(pcm), ptr(out), ptr(gain),
                                     ptr(vad), ptr(nse))
    check(lib, rc)
    res = [split(out, lens)] + [split(a, frames) for a in (gain, vad, nse) if a is not None]
    return res[0] if len(res) == 1 else tuple(res)


class LogmmseStream(Closing):
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
        rc, outs = stream_push(self._lib.bp_lmstream_push, self._s, self.n_chan, blocks, end, out_cap)
        check(self._lib, rc)
        return outs

    def close(self):
        if self._s is not None:
            self._lib.bp_lmstream_close(self._s)
        self._s = None


def logmmse_stream_open(device, fea_dim, params=None, n_chan=1, max_push_samples=16000, noise=None):
    """bp_lmstream_open: a LogmmseStream of n_chan channels on a device ordinal (params and noise as for logmmse_waves; noise
    other than None: bp_lmstream_open_nt)."""
    lib = load_library()
    lm = logmmse_params(params)
    s = C.c_void_p()
    if noise is None:
        rc = lib.bp_lmstream_open(int(device), int(fea_dim), _ref(lm), int(n_chan), int(max_push_samples), C.byref(s))
    else:
        nz = noise_params(noise)
        rc = lib.bp_lmstream_open_nt(int(device), int(fea_dim), _ref(lm), C.byref(nz), int(n_chan), int(max_push_samples), C.byref(s))
    check(lib, rc)
    if lm is None:
        lm = logmmse_params({})
    return LogmmseStream(lib, s, int(fea_dim), int(lm.init_frames), int(n_chan))


def logmmse_stream_counts(fea_dim, init_frames, received, ended):
    """bp_lmstream_counts: (frames_in, frames_out, samples_out) of a channel after `received` samples of its sentence; host only."""
    return _counts3("bp_lmstream_counts", int(fea_dim), int(init_frames), int(received), 1 if ended else 0)


def score_waves(device, fea_dim, sample_rate, refs, ests, extended=False):
    """bp_score_waves: SSNR, LSD and STOI of every estimate against its reference (lists of 1-D arrays, int16 units, pairwise
    equal lengths), float32 [n][3] (columns SCORE_SSNR, SCORE_LSD, SCORE_STOI; NaN where undefined).  No handle.  extended:
    bp_score_waves_ext, float32 [n][5] with SCORE_ESTOI and SCORE_SISDR behind the same three; extended="full": [n][7] with
    SCORE_LLR and SCORE_CD behind those five; extended="all": [n][9] with SCORE_FWSSNR and SCORE_WSS behind those seven
    (sample_rate from 8000 up).  Any other value is a BPError."""
    ns = score_columns("score_waves", extended)
    lib = load_library()
    if len(refs) != len(ests):
        raise BPError("score_waves: %d references but %d estimates" % (len(refs), len(ests)))
    rp, lens, _ = pack(refs)
    ep, elens, _ = pack(ests)
    bad = np.flatnonzero(lens != elens)
    if bad.size:
        raise BPError("score_waves: pair %d: reference has %d samples, estimate %d" % (bad[0], lens[bad[0]], elens[bad[0]]))
    n = len(lens)
    out = np.empty((max(n, 1), ns), np.float32)
    if ns != 3:
        rc = lib.bp_score_waves_ext(int(device), int(fea_dim), int(sample_rate), n, ptr(lens), ptr(rp), ptr(ep), ns, ptr(out))
    else:
        rc = lib.bp_score_waves(int(device), int(fea_dim), int(sample_rate), n, ptr(lens), ptr(rp), ptr(ep), ptr(out))
    check(lib, rc)
    return out[:n]


def resample_params(params=None):
    """None (the library's defaults: zeros 16, beta 8.6, rolloff 0.9), or a BPResampleParams: bp_resample_defaults overridden by
    the fields of a dict, or by a (zeros, beta, rolloff) tuple."""
    if params is None or isinstance(params, BPResampleParams):
        return params
    if not isinstance(params, dict):
        params = dict(zip(("zeros", "beta", "rolloff"), params))
    return struct_params(BPResampleParams, "bp_resample_defaults", "resample_params", params)


def resample_ratio(rate_in, rate_out):
    """bp_resample_ratio: (p, q) with rate_out / rate_in = p / q in lowest terms, max(p, q) <= 1024; host only."""
    lib = load_library()
    p, q = C.c_int(), C.c_int()
    check(lib, lib.bp_resample_ratio(int(rate_in), int(rate_out), C.byref(p), C.byref(q)))
    return int(p.value), int(q.value)


def resample_len(n, p, q):
    """bp_resample_len: ceil(n p / q), the samples a sentence of n samples becomes; host only."""
    lib = load_library()
    out = C.c_int64()
    check(lib, lib.bp_resample_len(int(n), int(p), int(q), C.byref(out)))
    return int(out.value)


def resample_taps(p, q, params=None):
    """bp_resample_taps: the 2 zeros max(p, q) + 1 float32 taps of the conversion by p / q; host only."""
    lib = load_library()
    rs = resample_params(params)
    zeros = 16 if rs is None else int(rs.zeros)
    h = np.empty(max(2 * max(zeros, 0) * max(int(p), int(q), 0) + 1, 1), np.float32)
    check(lib, lib.bp_resample_taps(int(p), int(q), _ref(rs), ptr(h), h.size))
    return h


def resample_waves(device, rate_in, rate_out, sentences, params=None):
    """bp_resample_waves: every sentence (1-D arrays) converted from rate_in to rate_out, a list of float32 arrays of
    resample_len samples each (no handle).  Defined to the bit in include/bp_c_api.h."""
    lib = load_library()
    rs = resample_params(params)
    p, q = resample_ratio(rate_in, rate_out)
    pcm, lens, _ = pack(sentences)
    n_out = (lens.astype(np.int64) * p + q - 1) // q
    out = np.empty(max(int(n_out.sum()), 1), np.float32)
    check(lib, lib.bp_resample_waves(int(device), int(rate_in), int(rate_out), _ref(rs), len(lens), ptr(lens), ptr(pcm), ptr(out)))
    return split(out, n_out)


def reverb_waves(device, sents, sent_rir, rirs, early_taps=0, early=True):
    """bp_reverb_waves: (rev, early) lists of the reverberant sentences and their direct-plus-early parts (None for early=False):
    sentence k convolved with rirs[sent_rir[k]], aligned to the direct path (include/bp_c_api.h).  No handle."""
    lib = load_library()
    spcm, slen, _ = pack(sents)
    hpcm, hlen, _ = pack(rirs)
    sr = np.ascontiguousarray(sent_rir, dtype=np.int32).reshape(-1)
    if sr.size != len(slen):
        raise BPError("reverb_waves: %d sentences but %d response indices" % (len(slen), sr.size))
    rev = np.empty(max(spcm.size, 1), np.float32)
    ear = np.empty(max(spcm.size, 1), np.float32) if early else None
    check(lib, lib.bp_reverb_waves(int(device), len(slen), ptr(slen), ptr(spcm), ptr(sr), len(hlen), ptr(hlen), ptr(hpcm),
                                   int(early_taps), ptr(rev), ptr(ear)))
    return split(rev, slen), (split(ear, slen) if early else None)


def rir_delay(h):
    """bp_mix_rir_delay: the first index at which |h[j]| is largest; host only."""
    lib = load_library()
    h = flat32(h)
    d = C.c_int()
    check(lib, lib.bp_mix_rir_delay(ptr(h) if h.size else None, h.size, C.byref(d)))
    return int(d.value)


def mix_reverb_pairs(seed, n_clean, n_rir):
    """bp_mix_reverb_pairs: the response of every clean sentence (int32 [n_clean]), keyed by the seed; host only."""
    lib = load_library()
    out = np.zeros(max(int(n_clean), 1), np.int32)
    check(lib, lib.bp_mix_reverb_pairs(int(seed), int(n_clean), int(n_rir), ptr(out)))
    return out[:int(n_clean)]


def _rooms(rooms):
    return np.ascontiguousarray(rooms, dtype=RIR_ROOM_DTYPE).reshape(-1)


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
    check(lib, lib.bp_rir_image(int(device), int(sample_rate), tw, int(r.size), r.ctypes.data_as(C.c_void_p) if r.size else None,
                                ptr(n) if n.size else None, ptr(out)))
    return split(out, n)


def rir_orders(room, sample_rate, n_taps, window_taps=None):
    """bp_rir_orders: ((N_0, N_1, N_2), images of the box) of one room; host only."""
    lib = load_library()
    r = _rooms(room)
    tw = rir_window_default(sample_rate) if window_taps is None else int(window_taps)
    order = np.zeros(3, np.int32)
    n = C.c_int64()
    check(lib, lib.bp_rir_orders(r.ctypes.data_as(C.c_void_p), int(sample_rate), int(n_taps), tw, ptr(order), C.byref(n)))
    return tuple(int(x) for x in order), int(n.value)


def rir_beta(L, t60):
    """bp_rir_beta: the six reflection coefficients (float64 [6]) Eyring's formula gives a box L for a NOMINAL t60; host only."""
    lib = load_library()
    Ld = np.ascontiguousarray(L, dtype=np.float64).reshape(-1)
    if Ld.size != 3:
        raise BPError("rir_beta: L needs 3 numbers")
    beta = np.zeros(6, np.float64)
    check(lib, lib.bp_rir_beta(ptr(Ld), float(t60), ptr(beta)))
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
    (t60_lo, t60_hi), (dist_lo, dist_hi) = g["t60"], g["dist"]
    set_fields(rg, "rir_rooms", dict(t60_lo=t60_lo, t60_hi=t60_hi, dist_lo=dist_lo, dist_hi=dist_hi, margin=g["margin"]))
    out = np.zeros(max(int(n), 1), RIR_ROOM_DTYPE)
    check(lib, lib.bp_rir_rooms(int(seed), int(n), C.byref(rg), out.ctypes.data_as(C.c_void_p)))
    return out[:int(n)]


def mix_plan(seed, n_clean, per_clean, noise_lens, snr_list):
    """bp_mix_plan: the shuffled mixture list (MIXTURE_DTYPE [n_clean * per_clean]); host only."""
    lib = load_library()
    nl = np.ascontiguousarray(noise_lens, dtype=np.int64)
    snr = np.ascontiguousarray(snr_list, dtype=np.float32)
    out = np.zeros(max(int(n_clean) * int(per_clean), 1), MIXTURE_DTYPE)
    check(lib, lib.bp_mix_plan(int(seed), int(n_clean), int(per_clean), nl.size, ptr(nl), snr.size, ptr(snr),
                               out.ctypes.data_as(C.c_void_p)))
    return out[:int(n_clean) * int(per_clean)]


def mix_shuffle(seed, stream, n):
    """bp_mix_shuffle: a permutation of range(n) (int32), keyed by (seed, stream); host only."""
    lib = load_library()
    out = np.zeros(max(int(n), 1), np.int32)
    check(lib, lib.bp_mix_shuffle(int(seed), int(stream), int(n), ptr(out)))
    return out[:int(n)]
