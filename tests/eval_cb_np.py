"""NumPy restatement of the two critical-band scores of the nine-column _ext calls (include/bp_c_api.h): the
frequency-weighted segmental SNR fwSegSNR (dB) and the weighted spectral slope distance WSS, on the segmental SNR's framing, over
25 Gaussian band filters on the n_fft-point spectra of the windowed frames.  Written from the definition in the header, not from
csrc/bp_eval.hip.  Everything runs in `dt` on the fp32 samples: np.float64 with numpy's FFT, np.longdouble with a direct DFT from
an 80-bit table (the precision check; slow, so on a subset of the frames) -- except Jk, which the definition computes in double.

The keyword switches of frame_values() and scores() are the wrong formulas of MUTANTS, which tests/test_eval_cb_host.py shows
the GPU bars to catch.  fixtures() makes the seeded signals both test files share: those of tests/eval_lpc_np.py and a few more."""
import math

import numpy as np

import eval_lpc_np as LP

BAR_FW, BAR_WSS = 1e-4, 1e-4                    # the GPU bars (absolute; fwSegSNR in dB)
NB = 25
CF = [50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30, 1288.72, 1442.54,
      1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63]
BW = [70.0] * 7 + [77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631,
                   255.255, 276.072, 298.126, 321.465, 346.136]
PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def framing(n, fs, skip_half=False):
    win = int(math.floor(0.03 * fs + 0.5))
    skip = win // 2 if skip_half else win // 4
    J = int(math.floor(n / skip - win / skip))
    return win, skip, max(J, 0)


def fft_size(win, short=False):
    """n_fft = 2^ceil(log2(2 win)); short (a mutant): 2^ceil(log2 win)"""
    n = 1
    while n < (win if short else 2 * win):
        n *= 2
    return n


def band_filters(fs, H, dt=np.float64, cut=True, floor_f0=True):
    """G[i][k], k < H: exp(-11 ((k - floor(f0_i)) / b_i)^2), zero where not above the cut"""
    k = np.arange(H).astype(dt)
    G = np.zeros((NB, H), dt)
    for i in range(NB):
        f0, b = dt(CF[i]) / (dt(fs) / 2) * H, dt(BW[i]) / (dt(fs) / 2) * H
        if floor_f0:
            f0 = np.floor(f0)
        G[i] = np.exp(-11 * ((k - f0) / b) ** 2)
    if cut:
        G[G <= np.exp(dt(-30) / (2 * dt("2.303")))] = 0
    return G


def cut_margin(fs, H):
    """the least relative distance of a filter value from the cut, over the table"""
    G = band_filters(fs, H, cut=False)
    c = math.exp(-30.0 / (2 * 2.303))
    return float(np.abs(G / c - 1).min())


def spectra(xw, n_fft, dt):
    """the bins 0 .. n_fft/2 - 1 of the n_fft-point DFT of every row of xw (zero-padded)"""
    H = n_fft // 2
    if dt == np.float64:
        return np.fft.rfft(xw, n_fft, axis=1)[:, :H]
    win = xw.shape[1]
    m = np.arange(n_fft).astype(dt)
    cs, sn = np.cos(2 * PI_LD * m / n_fft), np.sin(2 * PI_LD * m / n_fft)     # exp(-2 pi i m / n_fft) = cs - i sn
    idx = (np.arange(H)[:, None] * np.arange(win)[None, :]) % n_fft           # [k][n]
    return xw @ cs[idx].T - 1j * (xw @ sn[idx].T)


def nearest_peak(B, true_summit=False):
    """L[j][i], i < 24, by the search of the header; true_summit (a mutant): B_n on the rising side"""
    J = B.shape[0]
    ar = np.arange(J)
    s = B[:, 1:] - B[:, :-1]
    L = np.zeros((J, NB - 1), B.dtype)
    for i in range(NB - 1):
        up = s[:, i] > 0
        n = np.full(J, i)
        while True:
            go = up & (n < NB - 1) & (s[ar, np.minimum(n, NB - 2)] > 0)
            if not go.any():
                break
            n[go] += 1
        m = np.full(J, i)
        while True:
            go = ~up & (m >= 0) & (s[ar, np.maximum(m, 0)] <= 0)
            if not go.any():
                break
            m[go] -= 1
        rising = B[ar, n if true_summit else np.maximum(n - 1, 0)]
        L[:, i] = np.where(up, rising, B[ar, np.minimum(m + 1, NB - 1)])
    return L


def frame_values(r, e, fs, dt=np.float64, frames=None, gamma=0.2, swap_spectra=False, normalise=True, cut=True, floor_f0=True,
                 use_window=True, clamp=True, nfft_short=False, skip_half=False, kmax=20.0, true_summit=False, ref_weights=False,
                 floor=True):
    """(fwSegSNR_j, fw valid_j, WSS_j, WSS valid_j) over the J frames (frames: over that subset of them).  The keyword switches
    are the mutants."""
    r = np.asarray(r, np.float32).astype(dt)
    e = np.asarray(e, np.float32).astype(dt)
    win, skip, J = framing(r.size, fs, skip_half)
    js = np.arange(J) if frames is None else np.asarray(frames)
    if js.size == 0:
        return np.zeros(0, dt), np.zeros(0, bool), np.zeros(0, dt), np.zeros(0, bool)
    n_fft = fft_size(win, nfft_short)
    H = n_fft // 2
    w = LP.window(win, dt) if use_window else np.ones(win, dt)
    idx = js[:, None] * skip + np.arange(win)[None, :]
    rw, ew = w * r[idx], w * e[idx]
    valid = ((rw ** 2).sum(axis=1) > 0) & ((ew ** 2).sum(axis=1) > 0)
    G = band_filters(fs, H, dt, cut, floor_f0)
    with np.errstate(all="ignore"):             # (the invalid frames divide by zero: their values are never used)
        Rm, Em = np.abs(spectra(rw, n_fft, dt)).astype(dt), np.abs(spectra(ew, n_fft, dt)).astype(dt)
        Rp, Ep = Rm ** 2, Em ** 2
        if swap_spectra:
            Rm, Em, Rp, Ep = Rp, Ep, Rm, Em
        # fwSegSNR
        a, p = (Rm / Rm.sum(axis=1, keepdims=True), Em / Em.sum(axis=1, keepdims=True)) if normalise else (Rm, Em)
        c, d = a @ G.T, p @ G.T
        err = np.maximum((c - d) ** 2, dt(2.0) ** -52)
        pos = c > 0
        W = np.where(pos, c ** dt(gamma), 0)
        v = np.where(pos, W * 10 * np.log10(c * c / err), 0).sum(axis=1) / W.sum(axis=1)
        fvalid = valid & pos.any(axis=1)
        if clamp:
            v = np.clip(v, -10, 35)
        # WSS
        Bs, Cs = Rp @ G.T, Ep @ G.T
        if floor:
            Bs, Cs = np.maximum(Bs, dt("1e-10")), np.maximum(Cs, dt("1e-10"))
        B, C = 10 * np.log10(Bs), 10 * np.log10(Cs)
        s, t = B[:, 1:] - B[:, :-1], C[:, 1:] - C[:, :-1]
        kmax = dt(kmax)
        Wr = kmax / (kmax + B.max(axis=1, keepdims=True) - B[:, :-1]) * (1 / (1 + nearest_peak(B, true_summit) - B[:, :-1]))
        We = kmax / (kmax + C.max(axis=1, keepdims=True) - C[:, :-1]) * (1 / (1 + nearest_peak(C, true_summit) - C[:, :-1]))
        Ww = Wr if ref_weights else (Wr + We) / 2
        ws = (Ww * (s - t) ** 2).sum(axis=1) / Ww.sum(axis=1)
    return np.where(fvalid, v, 0), fvalid, np.where(valid, ws, 0), valid


def mean_of(v, valid, trim, rounded=True):
    """the mean over the valid frames, or (trim) over the lowest 95 % of them under eval_lpc_np.selected's rule"""
    sel = LP.selected(v, valid, trim)
    if sel.size == 0:
        return float("nan") if rounded else v.dtype.type("nan")
    m = v[sel].sum() / v.dtype.type(sel.size)
    return float(np.float32(m)) if rounded else m


def scores(r, e, fs, dt=np.float64, rounded=True, trim_fw=False, trim_wss=True, **kw):
    """(fwSegSNR, WSS) of a pair, rounded once to fp32 as the library rounds; rounded=False: in dt"""
    fw, fv, ws, wv = frame_values(r, e, fs, dt, **kw)
    return mean_of(fw, fv, trim_fw, rounded), mean_of(ws, wv, trim_wss, rounded)


def clamped_share(r, e, fs):
    """the share of the valid frames that a clamp of fwSegSNR holds"""
    fw, fv, _, _ = frame_values(r, e, fs, clamp=False)
    return float(((fw[fv] < -10) | (fw[fv] > 35)).sum()) / max(int(fv.sum()), 1)


# name -> (keywords of scores, the main fixture that catches it, which measure there)
MUTANTS = {
    "gamma_1": (dict(gamma=1.0), "rev8", "fw"),
    "spectra_swapped_fw": (dict(swap_spectra=True), "rev8", "fw"),
    "spectra_swapped_wss": (dict(swap_spectra=True), "rev8", "wss"),
    "no_normalisation": (dict(normalise=False), "rev8", "fw"),
    "no_cut": (dict(cut=False), "rev16", "wss"),
    "f0_not_floored": (dict(floor_f0=False), "rev8", "wss"),
    "no_window": (dict(use_window=False), "rev16", "wss"),
    "no_clamp": (dict(clamp=False), "rev8", "fw"),
    "nfft_short": (dict(nfft_short=True), "rev8", "wss"),
    "skip_half": (dict(skip_half=True), "rev8", "wss"),
    "kmax_1": (dict(kmax=1.0), "rev8", "wss"),
    "true_summit": (dict(true_summit=True), "rev8", "wss"),
    "reference_weights": (dict(ref_weights=True), "rev8", "wss"),
    "no_trim_wss": (dict(trim_wss=False), "burst8", "wss"),
    "trim_fw": (dict(trim_fw=True), "rev8", "fw"),
    "no_floor": (dict(floor=False), "faint8", "wss"),
}


def fixtures():
    """{name: (fs, r, e, kind)}: those of eval_lpc_np.fixtures(), a 15 dB pair and a pair with faint stretches per rate, and one
    pair at 48 kHz and one at 80 kHz (n_fft 4096 / 8192).  kind "main": a pair the parity bars and the mutants are judged on;
    "clamp": the 30 dB and burst pairs, which sit on fwSegSNR's upper clamp (main pairs for WSS alone); "edge": exercised only.  Seeded; made once, read only."""
    out = {}
    for name, (fs, r, e, kind) in LP.fixtures().items():
        if name.startswith("snr5_"):
            kind = "main"
        elif name.startswith(("snr30_", "burst")):
            kind = "clamp"
        out[name] = (fs, r, e, kind)
    for fs, tag in ((8000, "8"), (16000, "16")):
        rng = np.random.default_rng(5100 + fs)
        r = out["rev" + tag][1]
        out["snr15_" + tag] = (fs, r, LP.add_noise(rng, r, 15.0), "main")
        # the silent segments of the reference filled with noise far below the 1e-10 floor of the band energies, in both signals
        quiet = r == 0.0
        fr = r.copy()
        fr[quiet] = (1e-9 * rng.normal(size=int(quiet.sum()))).astype(np.float32)
        fe = LP.add_noise(rng, r, 15.0)
        fe[quiet] = (1e-9 * rng.normal(size=int(quiet.sum()))).astype(np.float32)
        out["faint" + tag] = (fs, fr, fe, "main")
    for fs, sec in ((48000, 0.3), (80000, 0.25)):
        rng = np.random.default_rng(5200 + fs)
        r = LP.speech_like(rng, fs, sec=sec)
        out["wide%d" % (fs // 1000)] = (fs, r, LP.add_noise(rng, r, 15.0), "main")
    return out
