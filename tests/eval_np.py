"""NumPy restatement of the objective scores of bp_score_waves / bp_eval_mix (include/bp_c_api.h), in float64:
the segmental SNR of Hu & Loizou, the log-spectral distortion on the 1d analysis, and STOI (Taal et al. 2011, with pystoi's
guards) with scipy's resample_poly restated.  Written from the definitions, not from csrc/bp_eval.hip; no scipy.  Also the test
signals: harmonic tones under a syllable-rate envelope, exact-zero gaps and a broadband floor."""
import math

import numpy as np

import wave_np as WN

EPS = 2.220446049250313e-16
N_FRAME, HOP, NFFT, N_SEG = 256, 128, 512, 30
BANDS = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219)]


def rate_pq(fs):
    """10000/fs = p/q in lowest terms, or None when the rate is not accepted."""
    if fs <= 0:
        return None
    g = math.gcd(10000, int(fs))
    p, q = 10000 // g, int(fs) // g
    return (p, q) if max(p, q) <= 32 else None


def thirdoct(fs=10000, nfft=NFFT, num_bands=15, min_freq=150):
    """The MATLAB thirdoct nearest-bin rule: [lo, hi) bin ranges of the one-third-octave bands."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    fl = np.sqrt((2.0 ** (k / 3) * min_freq) * 2.0 ** ((k - 1) / 3) * min_freq)
    fr = np.sqrt((2.0 ** (k / 3) * min_freq) * 2.0 ** ((k + 1) / 3) * min_freq)
    return [(int(np.argmin((f - fl[i]) ** 2)), int(np.argmin((f - fr[i]) ** 2))) for i in range(num_bands)]


def resample_taps(p, q):
    m = max(p, q)
    Lh = 10 * m
    j = np.arange(2 * Lh + 1)
    h = np.kaiser(2 * Lh + 1, 5.0) * np.sinc((j - Lh) / m)
    return h / h.sum() * p, Lh


def resample(x, fs):
    """x at fs -> 10 kHz: y[k] = sum_j h[j] u[k q + Lh - j], u = x upsampled by p with zeros, k < ceil(n p / q)."""
    x = np.asarray(x, np.float64)
    p, q = rate_pq(fs)
    if p == 1 and q == 1:
        return x.copy()
    h, Lh = resample_taps(p, q)
    u = np.zeros(x.size * p)
    u[::p] = x
    full = np.convolve(u, h)
    n10 = -(-x.size * p // q)
    return full[np.arange(n10) * q + Lh]


def ssnr_frames(r, e, fs):
    r = np.asarray(r, np.float64)
    e = np.asarray(e, np.float64)
    win = int(math.floor(0.03 * fs + 0.5))
    skip = win // 4
    J = int(math.floor(r.size / skip - win / skip))
    if J < 1:
        return np.zeros(0)
    w = 0.5 * (1 - np.cos(2 * np.pi * (np.arange(win) + 1) / (win + 1)))
    idx = np.arange(J)[:, None] * skip + np.arange(win)[None, :]
    Es = ((w * r[idx]) ** 2).sum(axis=1)
    Ed = ((w * (r[idx] - e[idx])) ** 2).sum(axis=1)
    return np.clip(10 * np.log10(Es / (Ed + EPS) + EPS), -10.0, 35.0)


def ssnr(r, e, fs):
    s = ssnr_frames(r, e, fs)
    return float(s.mean()) if s.size else float("nan")


def lsd_of_lps(Lr, Le):
    d = (10.0 / np.log(10.0)) * (np.asarray(Lr, np.float64) - np.asarray(Le, np.float64))
    return float(np.sqrt((d ** 2).mean(axis=1)).mean())


def lsd(r, e, fea_dim):
    return lsd_of_lps(WN.lps(WN.analysis(r, fea_dim)), WN.lps(WN.analysis(e, fea_dim)))


def stoi_window():
    return 0.5 * (1 - np.cos(2 * np.pi * (np.arange(N_FRAME) + 1) / (N_FRAME + 1)))


def frame_energies(r10):
    v = stoi_window()
    starts = np.arange(0, r10.size - N_FRAME, HOP)
    return np.array([((v * r10[s:s + N_FRAME]) ** 2).sum() for s in starts])


def mask_margin(r, fs):
    """Smallest |E_j - thr| / thr over the STOI frames of r (inf without frames or with a silent r)."""
    E = frame_energies(resample(r, fs))
    if E.size == 0 or E.max() == 0:
        return float("inf")
    thr = 1e-4 * E.max()
    return float(np.min(np.abs(E - thr)) / thr)


def stoi(r, e, fs, check_margin=False):
    r10, e10 = resample(r, fs), resample(e, fs)
    v = stoi_window()
    E = frame_energies(r10)
    if E.size == 0:
        return float("nan")
    thr = 1e-4 * E.max()
    if check_margin and E.max() > 0:
        assert np.all(np.abs(E - thr) > 0.01 * thr), "a frame energy lies within 1 % of the threshold"
    kept = np.nonzero(E > thr)[0]
    C = kept.size
    if C < 1:
        return float("nan")
    rc = np.zeros((C - 1) * HOP + N_FRAME)
    ec = np.zeros_like(rc)
    for c, j in enumerate(kept):
        rc[c * HOP:c * HOP + N_FRAME] += v * r10[j * HOP:j * HOP + N_FRAME]
        ec[c * HOP:c * HOP + N_FRAME] += v * e10[j * HOP:j * HOP + N_FRAME]
    starts = np.arange(0, rc.size - N_FRAME, HOP)
    S = starts.size
    assert S == C - 1
    if S < N_SEG:
        return float("nan")

    def bands(x):
        P = np.abs(np.fft.rfft(np.stack([v * x[s:s + N_FRAME] for s in starts]), n=NFFT, axis=1)) ** 2
        return np.stack([np.sqrt(P[:, a:b].sum(axis=1)) for a, b in BANDS], axis=1)   # [S][15]

    X, Y = bands(rc), bands(ec)
    clip = 1 + 10 ** 0.75
    rho = []
    for m in range(N_SEG - 1, S):
        x, y = X[m - N_SEG + 1:m + 1], Y[m - N_SEG + 1:m + 1]                          # [30][15]
        al = np.sqrt((x ** 2).sum(axis=0) / ((y ** 2).sum(axis=0) + EPS))
        yp = np.minimum(al * y, clip * x)
        dx, dy = x - x.mean(axis=0), yp - yp.mean(axis=0)
        rho.append((dx * dy).sum(axis=0) / ((np.sqrt((dx ** 2).sum(axis=0)) + EPS) * (np.sqrt((dy ** 2).sum(axis=0)) + EPS)))
    return float(np.mean(rho))


def scores(r, e, fs, fea_dim, check_margin=False):
    return np.array([ssnr(r, e, fs), lsd(r, e, fea_dim), stoi(r, e, fs, check_margin)])


# ---- test signals
def speech_like(rng, n, fs, peak=8000.0, floor_db=-35.0, gaps=2, f0=130.0):
    """Harmonic tones (to 3.5 kHz) under a syllable-rate envelope, `gaps` exact-zero gaps of 0.15 s, and a white floor
    floor_db below the peak everywhere outside the gaps.  float32, int16 units.  The gaps are moved until no STOI frame energy
    lies within 5 % of the 40 dB threshold."""
    t = np.arange(n) / fs
    ph = 2 * np.pi * np.cumsum(f0 * (1 + 0.1 * np.sin(2 * np.pi * 0.7 * t))) / fs
    nh = max(1, int(min(3500.0, 0.45 * fs) // (1.1 * f0)))
    tone = sum(np.sin(h * ph + rng.uniform(0, 2 * np.pi)) / h for h in range(1, nh + 1))
    env = 0.15 + 0.85 * np.abs(np.sin(2 * np.pi * 2.3 * t + rng.uniform(0, np.pi)))
    x = env * tone
    x = x / np.abs(x).max() * peak + rng.normal(0.0, peak * 10 ** (floor_db / 20), n)
    x = x.astype(np.float32)
    if gaps == 0:
        return x
    g = int(0.15 * fs)
    for shift in range(64):
        y = x.copy()
        for k in range(gaps):
            a = int((k + 1) * n / (gaps + 1)) + shift * (fs // 997)
            y[a:a + g] = 0.0
        if mask_margin(y, fs) > 0.05:
            return y
    raise AssertionError("no gap placement keeps the STOI frames away from the threshold")


def add_noise(rng, r, snr_db):
    r = np.asarray(r, np.float64)
    n = rng.normal(0.0, 1.0, r.size)
    n *= np.sqrt((r ** 2).sum() / ((n ** 2).sum() * 10 ** (snr_db / 10)))
    return (r + n).astype(np.float32)
