"""NumPy restatement of the two extended scores of bp_score_waves_ext / bp_eval_mix_ext (include/bp_c_api.h), in
float64: ESTOI (Jensen & Taal 2016, without the random dither) and SI-SDR (Le Roux et al. 2019).  The STOI front end -- resampler,
40 dB frame removal, compaction, one-third-octave envelopes -- is restated from tests/eval_np.py's own helpers, because its stoi()
does not hand out the envelopes; stoi_from_front() puts STOI's own correlation step behind that front end, and
tests/test_eval_ext_host.py holds it equal to eval_np.stoi.  Written from the definitions, not from csrc/bp_eval.hip.  The keyword
switches of estoi() and sisdr() are the wrong formulas that the host test shows the GPU bars to catch."""
import math

import numpy as np

import eval_np as EN

EPS = EN.EPS
N_FRAME, HOP, NFFT, N_SEG = EN.N_FRAME, EN.HOP, EN.NFFT, EN.N_SEG


def front(r, e, fs, check_margin=False):
    """The envelopes (X, Y), each [S][15], of reference and estimate; None where STOI and ESTOI are undefined (no frame, no kept
    frame, S < 30)."""
    r10, e10 = EN.resample(r, fs), EN.resample(e, fs)
    v = EN.stoi_window()
    E = EN.frame_energies(r10)
    if E.size == 0:
        return None
    thr = 1e-4 * E.max()
    if check_margin and E.max() > 0:
        assert np.all(np.abs(E - thr) > 0.01 * thr), "a frame energy lies within 1 % of the threshold"
    kept = np.nonzero(E > thr)[0]
    C = kept.size
    if C < 1:
        return None
    rc = np.zeros((C - 1) * HOP + N_FRAME)
    ec = np.zeros_like(rc)
    for c, j in enumerate(kept):
        rc[c * HOP:c * HOP + N_FRAME] += v * r10[j * HOP:j * HOP + N_FRAME]
        ec[c * HOP:c * HOP + N_FRAME] += v * e10[j * HOP:j * HOP + N_FRAME]
    starts = np.arange(0, rc.size - N_FRAME, HOP)
    if starts.size < N_SEG:
        return None

    def bands(x):
        P = np.abs(np.fft.rfft(np.stack([v * x[s:s + N_FRAME] for s in starts]), n=NFFT, axis=1)) ** 2
        return np.stack([np.sqrt(P[:, a:b].sum(axis=1)) for a, b in EN.BANDS], axis=1)

    return bands(rc), bands(ec)


def _clipped(x, y):
    """STOI's scale-and-clip of a [30][15] segment of the estimate."""
    al = np.sqrt((x ** 2).sum(axis=0) / ((y ** 2).sum(axis=0) + EPS))
    return np.minimum(al * y, (1 + 10 ** 0.75) * x)


def stoi_from_front(r, e, fs, check_margin=False):
    """STOI's correlation step (eval_np.stoi's, line for line) on front()'s envelopes."""
    f = front(r, e, fs, check_margin)
    if f is None:
        return float("nan")
    X, Y = f
    rho = []
    for m in range(N_SEG - 1, X.shape[0]):
        x, y = X[m - N_SEG + 1:m + 1], Y[m - N_SEG + 1:m + 1]
        yp = _clipped(x, y)
        dx, dy = x - x.mean(axis=0), yp - yp.mean(axis=0)
        rho.append((dx * dy).sum(axis=0) / ((np.sqrt((dx ** 2).sum(axis=0)) + EPS) * (np.sqrt((dy ** 2).sum(axis=0)) + EPS)))
    return float(np.mean(rho))


def _normalise(a, rows=True, cols=True):
    """a: [15][30], bands by frames.  Rows (each band over the 30 frames), then columns (each frame over the 15 bands)."""
    if rows:
        a = a - a.mean(axis=1, keepdims=True)
        a = a / (np.sqrt((a ** 2).sum(axis=1, keepdims=True)) + EPS)
    if cols:
        a = a - a.mean(axis=0, keepdims=True)
        a = a / (np.sqrt((a ** 2).sum(axis=0, keepdims=True)) + EPS)
    return a


def estoi(r, e, fs, check_margin=False, rows=True, cols=True, clip=False):
    """ESTOI.  The mutants: rows=False, cols=False leave a normalisation step out; clip=True puts STOI's scale-and-clip in front."""
    f = front(r, e, fs, check_margin)
    if f is None:
        return float("nan")
    X, Y = f
    d = []
    for m in range(N_SEG - 1, X.shape[0]):
        x, y = X[m - N_SEG + 1:m + 1], Y[m - N_SEG + 1:m + 1]                          # [30][15]
        if clip:
            y = _clipped(x, y)
        d.append((_normalise(x.T, rows, cols) * _normalise(y.T, rows, cols)).sum() / N_SEG)
    return float(np.mean(d))


def sisdr(r, e, unit_alpha=False, remove_mean=False):
    """SI-SDR in dB.  The mutants: unit_alpha=True is the plain SDR (alpha = 1), remove_mean=True takes the means out first."""
    r = np.asarray(r, np.float64)
    e = np.asarray(e, np.float64)
    if remove_mean:
        r, e = r - r.mean(), e - e.mean()
    rr, er = (r * r).sum(), (e * r).sum()
    if rr == 0:
        return float("nan")
    al = 1.0 if unit_alpha else er / rr
    num, den = ((al * r) ** 2).sum(), ((al * r - e) ** 2).sum()
    return float(10 * math.log10(num / (den + EPS) + EPS))


def scores5(r, e, fs, fea_dim, check_margin=False):
    return np.concatenate([EN.scores(r, e, fs, fea_dim, check_margin), [estoi(r, e, fs, check_margin), sisdr(r, e)]])


def pair_set(rng, fs):
    """The pairs the extended scores are tested on: speech_like references of 3.0, 2.5 and 4.0 s with white noise at 0, 10 and
    20 dB (pairs 0..2, the SNR rising), 0.5 (r + noise) of pair 0 (pair 3: a pure gain change), and pair 1's estimate with an
    offset of 100 (pair 4: speech_like and white noise have next to no mean, so that without it nothing would tell an SI-SDR
    that removes the means from one that does not)."""
    refs = [EN.speech_like(rng, int(sec * fs), fs) for sec in (3.0, 2.5, 4.0)]
    ests = [EN.add_noise(rng, r, snr) for r, snr in zip(refs, (0.0, 10.0, 20.0))]
    return refs + [refs[0], refs[1]], ests + [(0.5 * ests[0]).astype(np.float32), (ests[1] + 100.0).astype(np.float32)]
