"""NumPy restatement of the two spectral-envelope scores of the seven-column _ext calls (include/bp_c_api.h):
the log-likelihood ratio LLR and the LPC cepstral distance CD in dB (Hu & Loizou 2008), on the segmental SNR's framing, with the
white-noise correction of R[0] and the mean of the lowest 95 % of the valid frames under the stated tie rule.  Written from the
definition in the header, not from csrc/bp_eval.hip.  Everything runs in `dt` (np.float64; np.longdouble for the precision
check) on the fp32 samples -- except Jk, which the definition computes in double and which therefore stays a Python float.

The keyword switches of frame_values() and lowest_mean() are the wrong formulas of MUTANTS, which tests/test_eval_lpc_host.py
shows the GPU bars to catch.  fixtures() makes the seeded signals both test files share."""
import math

import numpy as np

WNC = 1e-6                                      # R[0] <- R[0] (1 + WNC)
BAR_LLR, BAR_CD = 1e-5, 1e-4                    # the GPU bars (absolute; CD in dB)


def framing(n, fs):
    win = int(math.floor(0.03 * fs + 0.5))
    skip = win // 4
    J = int(math.floor(n / skip - win / skip))
    return win, skip, max(J, 0)


def order(fs):
    return 10 if fs < 10000 else 16


def window(win, dt=np.float64):
    return (0.5 * (1 - np.cos(2 * np.pi * (np.arange(win) + 1) / (win + 1)))).astype(dt)   # (the library's table is a double)


def autocorr(xw, P):
    """R[j][k] = sum_{i=0}^{win-1-k} xw[j][i] xw[j][i+k], k = 0..P"""
    win = xw.shape[1]
    return np.stack([(xw[:, :win - k] * xw[:, k:]).sum(axis=1) for k in range(P + 1)], axis=1)


def levinson(R, P):
    """a[j][1..P] of every row of R (index 0 unused): the recursion of the header, line for line."""
    J, dt = R.shape[0], R.dtype
    a = np.zeros((J, P + 1), dt)
    E = R[:, 0].copy()
    for m in range(1, P + 1):
        s = np.zeros(J, dt)
        for j in range(1, m):
            s = s + a[:, j] * R[:, m - j]
        k = (R[:, m] - s) / E
        new = a.copy()
        new[:, m] = k
        for j in range(1, m):
            new[:, j] = a[:, j] - k * a[:, m - j]
        a = new
        E = (1 - k * k) * E
    return a


def cepstrum(a, P, weight=True):
    """c_1 = a_1, c_m = a_m + sum_{q<m} (q/m) c_q a_{m-q}; weight=False (a mutant) drops q/m."""
    c = np.zeros_like(a)
    c[:, 1] = a[:, 1]
    for m in range(2, P + 1):
        s = np.zeros(a.shape[0], a.dtype)
        for q in range(1, m):
            s = s + (a.dtype.type(q) / a.dtype.type(m) if weight else a.dtype.type(1)) * c[:, q] * a[:, m - q]
        c[:, m] = a[:, m] + s
    return c


def quad(A, R):
    """A T A^T per row, T the Toeplitz matrix of the row of R"""
    n = R.shape[1]
    idx = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    return np.einsum("ji,jik,jk->j", A, R[:, idx], A)


def frame_values(r, e, fs, dt=np.float64, p_off=0, use_window=True, clamp=True, wnc=WNC, swap=False, t_from_e=False, cep_weight=True):
    """(LLR_j, CD_j, valid_j) over the J frames.  The keyword switches are the mutants."""
    r = np.asarray(r, np.float32).astype(dt)
    e = np.asarray(e, np.float32).astype(dt)
    win, skip, J = framing(r.size, fs)
    if J < 1:
        return np.zeros(0, dt), np.zeros(0, dt), np.zeros(0, bool)
    P = order(fs) + p_off
    w = window(win, dt) if use_window else np.ones(win, dt)
    idx = np.arange(J)[:, None] * skip + np.arange(win)[None, :]
    Rr, Re = autocorr(w * r[idx], P), autocorr(w * e[idx], P)
    valid = (Rr[:, 0] > 0) & (Re[:, 0] > 0)
    Rr[:, 0] = Rr[:, 0] * (1 + dt(wnc))
    Re[:, 0] = Re[:, 0] * (1 + dt(wnc))
    with np.errstate(all="ignore"):             # (the invalid frames divide by zero: their values are never used)
        ar, ae = levinson(Rr, P), levinson(Re, P)
        cr, ce = cepstrum(ar, P, cep_weight), cepstrum(ae, P, cep_weight)
        Ar, Ae = -ar, -ae
        Ar[:, 0] = Ae[:, 0] = 1
        if swap:
            Ar, Ae = Ae, Ar
        T = Re if t_from_e else Rr
        llr = np.log(quad(Ae, T) / quad(Ar, T))
        cd = (10 / np.log(dt(10))) * np.sqrt(2 * ((cr[:, 1:] - ce[:, 1:]) ** 2).sum(axis=1))
    if clamp:
        llr, cd = np.clip(llr, 0, 2), np.clip(cd, 0, 10)
    llr, cd = np.where(valid, llr, 0), np.where(valid, cd, 0)
    return llr, cd, valid


def keep(Jv):
    return max(1, int(math.floor(0.95 * Jv + 0.5)))


def selected(v, valid, trim=True, ties="low_index_first"):
    """the frame indices the score sums: rank #{valid i: v_i < v_j, or v_i == v_j and i < j} below Jk; trim=False (a mutant)
    keeps every valid frame; ties (mutants): "high_index_first" (i > j), "unbroken" (every equal frame counts)"""
    ix = np.nonzero(valid)[0]
    if ix.size == 0:
        return ix
    x = v[ix]
    Jk = keep(ix.size) if trim else ix.size
    first = {"low_index_first": ix[:, None] < ix[None, :], "high_index_first": ix[:, None] > ix[None, :],
             "unbroken": ix[:, None] != ix[None, :]}[ties]                                     # [i][j]: i counts against j among equals
    rank = ((x[:, None] < x[None, :]) | ((x[:, None] == x[None, :]) & first)).sum(axis=0)
    return ix[rank < Jk]


def lowest_mean(v, valid, trim=True, ties="low_index_first"):
    sel = selected(v, valid, trim, ties)
    if sel.size == 0:
        return float("nan")
    return float(np.float32(v[sel].sum() / v.dtype.type(sel.size)))


def llr_cd(r, e, fs, dt=np.float64, trim=True, ties="low_index_first", rounded=True, **kw):
    """(LLR, CD) of a pair, rounded once to fp32 as the library rounds; rounded=False: in dt (the precision check)"""
    llr, cd, valid = frame_values(r, e, fs, dt, **kw)
    if rounded:
        return lowest_mean(llr, valid, trim, ties), lowest_mean(cd, valid, trim, ties)
    out = []
    for v in (llr, cd):
        sel = selected(v, valid, trim, ties)
        out.append(v[sel].sum() / dt(sel.size) if sel.size else dt("nan"))
    return tuple(out)


def clamped_share(r, e, fs):
    """the share of the valid frames that either clamp holds, per measure"""
    llr, cd, valid = frame_values(r, e, fs, clamp=False)
    n = max(int(valid.sum()), 1)
    return float(((llr[valid] < 0) | (llr[valid] > 2)).sum()) / n, float(((cd[valid] < 0) | (cd[valid] > 10)).sum()) / n


# name -> (keywords of llr_cd, the main fixture that catches it, which measure there).  ties="high_index_first" has no row: see
# tests/test_eval_lpc_host.py::test_reversed_tie_order_moves_the_frames_but_no_score
MUTANTS = {
    "P_plus_1": (dict(p_off=1), "rev8", "cd"),
    "P_minus_1": (dict(p_off=-1), "rev8", "cd"),
    "no_window": (dict(use_window=False), "rev16", "llr"),
    "no_trim": (dict(trim=False), "rev8", "llr"),
    "no_clamp": (dict(clamp=False), "burst8", "llr"),
    "correction_omitted": (dict(wnc=0.0), "tones16", "llr"),
    "correction_1e-4": (dict(wnc=1e-4), "rev16", "llr"),
    "A_swapped": (dict(swap=True), "rev8", "llr"),
    "T_from_R_e": (dict(t_from_e=True), "rev8", "llr"),
    "cepstrum_unweighted": (dict(cep_weight=False), "rev8", "cd"),
    "ties_unbroken": (dict(ties="unbroken"), "burst8", "llr"),
}


# ---- the signals
def _resonate(x, fs, freqs, bws):
    """x through a cascade of two-pole resonators (a plain recursion in double)"""
    y = np.asarray(x, np.float64)
    for f, bw in zip(freqs, bws):
        rad = math.exp(-math.pi * bw / fs)
        b1, b2 = 2 * rad * math.cos(2 * math.pi * f / fs), -rad * rad
        out = np.zeros_like(y)
        y1 = y2 = 0.0
        for i in range(y.size):
            v = y[i] + b1 * y1 + b2 * y2
            out[i] = v
            y2, y1 = y1, v
        y = out
    return y


def speech_like(rng, fs, sec=2.0, peak=8000.0):
    """Segments of 0.2 s: pulse-excited (voiced), noise-excited (unvoiced) or exactly silent, each through its own three formants.
    The formants are those of 8 kHz speech scaled by fs / 8000, so that they fill the band at every rate: above a band-limited
    reference any white noise is the whole signal, and every frame would sit on the clamps.  float32, int16 units."""
    n, seg = int(sec * fs), int(0.2 * fs)
    x = np.zeros(n)
    kinds = ["v", "n", "v", "s", "n", "v", "v", "s", "n", "v"]
    for k, a in enumerate(range(0, n, seg)):
        kind = kinds[k % len(kinds)]
        m = min(seg, n - a)
        if kind == "s":
            continue
        if kind == "v":
            exc = np.zeros(m)
            exc[::int(fs / rng.uniform(100.0, 180.0))] = 1.0
            exc += 0.01 * rng.normal(size=m)
        else:
            exc = rng.normal(size=m)
        f = [rng.uniform(300, 800) * fs / 8000, rng.uniform(1000, 2200) * fs / 8000, rng.uniform(2500, 3400) * fs / 8000]
        y = _resonate(exc, fs, f, [80.0 * fs / 8000, 120.0 * fs / 8000, 160.0 * fs / 8000]) * np.hanning(m + 2)[1:-1] ** 0.25
        x[a:a + m] = y / np.abs(y).max() * rng.uniform(0.3, 1.0)
    return (x * peak).astype(np.float32)


def reverberate(rng, r, fs, ms):
    """r through a decaying-noise FIR of `ms` milliseconds (60 dB down at its end), the direct sound in front"""
    L = int(ms * 1e-3 * fs)
    h = rng.normal(size=L) * 10 ** (-3.0 * np.arange(L) / L)
    h[0] = 1.0
    h[1:] *= 0.5 / np.sqrt((h[1:] ** 2).sum())
    return np.convolve(np.asarray(r, np.float64), h)[:r.size].astype(np.float32)


def add_noise(rng, r, snr_db):
    r = np.asarray(r, np.float64)
    n = rng.normal(size=r.size)
    n *= np.sqrt((r ** 2).sum() / ((n ** 2).sum() * 10 ** (snr_db / 10)))
    return (r + n).astype(np.float32)


def tones(rng, fs, noise_db, sec=1.0, peak=8000.0):
    """a few steady tones plus white noise noise_db below them: an autocorrelation matrix so close to singular that the
    white-noise correction decides the result"""
    t = np.arange(int(sec * fs)) / fs
    x = sum(np.sin(2 * np.pi * f * t + p) for f, p in zip((440.0, 1130.0, 2310.0), (0.3, 1.1, 2.0)))
    x = x / np.abs(x).max()
    return (peak * (x + 10 ** (noise_db / 20) * rng.normal(size=t.size))).astype(np.float32)


def fixtures():
    """{name: (fs, r, e, kind)}; kind "main": a pair the parity bars and the mutants are judged on; "edge": exercised only.
    Seeded; made once by the callers and read only."""
    out = {}
    for fs, tag in ((8000, "8"), (16000, "16")):
        rng = np.random.default_rng(4100 + fs)
        r = speech_like(rng, fs)
        out["rev" + tag] = (fs, r, reverberate(rng, r, fs, 100.0 if fs == 8000 else 200.0), "main")
        out["snr30_" + tag] = (fs, r, add_noise(rng, r, 30.0), "main")
        b = add_noise(rng, r, 30.0).astype(np.float64)                      # a burst of loud noise: 5 .. 10 % of the frames on the upper clamps,
        a, m = int(0.45 * fs), int((0.10 if fs == 8000 else 0.13) * fs)     # more than the trim drops, so that the clamps and the tie rule count
        b[a:a + m] += rng.normal(size=m) * 30.0 * np.sqrt((r[a:a + m].astype(np.float64) ** 2).mean())
        out["burst" + tag] = (fs, r, b.astype(np.float32), "main")
        out["same" + tag] = (fs, r, r.copy(), "edge")
        out["zeros" + tag] = (fs, r, np.zeros_like(r), "edge")
        out["snr5_" + tag] = (fs, r, add_noise(rng, r, 5.0), "edge")         # (kept only to exercise the clamps)
        lead = r.copy()
        lead[:int(0.1 * fs)] = 0.0
        out["lead" + tag] = (fs, lead, add_noise(rng, lead, 30.0), "edge")   # an exact-zero lead: invalid frames are skipped
        win, skip, _ = framing(r.size, fs)
        a = int(0.05 * fs)
        for name, n in (("short", win - 1), ("noframe", win + skip - 1), ("oneframe", win + skip), ("jv10_", win + 10 * skip),
                        ("jv11_", win + 11 * skip)):
            x = r[a:a + n]
            out[name + tag] = (fs, x, add_noise(rng, x, 30.0), "edge")
        t = np.random.default_rng(4200 + fs)
        out["tones" + tag] = (fs, tones(t, fs, -50.0), tones(t, fs, -40.0), "main")
    return out
