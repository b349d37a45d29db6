"""NumPy restatement of the log-MMSE baseline enhancer (bp_logmmse_waves, include/bp_c_api.h), in float64 and
from the PCM samples on: its own analysis, exponential integral, recursion and least-squares overlap-add.  Written from the
definition; it calls nothing in the library.  Also the fixture sentences that tests/test_classic_host.py vets and
tests/test_classic_gpu.py runs: gated tones in white noise behind a noise-only lead, and the edge cases."""
import numpy as np

DEFAULTS = dict(alpha=0.98, mu=0.98, eta=0.15, xi_min_db=-25.0, gamma_max=40.0, init_frames=6)
ALT = dict(alpha=0.95, mu=0.9, eta=0.2, xi_min_db=-15.0, gamma_max=20.0, init_frames=4)   # the non-default set of the tests
LAMBDA_FLOOR = 1e-10
EULER = 0.57721566490153286061


# ---- the signal definition
def geometry(fea_dim):
    n_fft = 2 * (fea_dim - 1)
    return n_fft, n_fft // 2


def n_frames(n, fea_dim):
    return (n - 1) // (fea_dim - 1) + 2


def window(n_fft):
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def analysis(x, fea_dim):
    """Y [T][fea_dim] complex128: n_fft - hop zeros in front, zeros behind, T = (n-1)/hop + 2 frames of the periodic Hamming window."""
    n_fft, hop = geometry(fea_dim)
    x = np.asarray(x, np.float64)
    T = n_frames(x.size, fea_dim)
    xp = np.zeros((T + 1) * hop)
    xp[hop:hop + x.size] = x
    w = window(n_fft)
    return np.stack([np.fft.rfft(xp[t * hop:t * hop + n_fft] * w) for t in range(T)])


def overlap_add(S, n):
    """sum_t w irfft(S_t) / sum_t w^2 over the frames that cover a sample, trimmed to n samples."""
    T, D = S.shape
    n_fft, hop = geometry(D)
    w = window(n_fft)
    num = np.zeros((T + 1) * hop)
    den = np.zeros((T + 1) * hop)
    for t in range(T):
        num[t * hop:t * hop + n_fft] += w * np.fft.irfft(S[t], n=n_fft)
        den[t * hop:t * hop + n_fft] += w * w
    return (num / den)[hop:hop + n]


# ---- the exponential integral
def e1_series(x):
    """-gamma_E - ln x - sum_{n>=1} (-x)^n / (n n!), summed until the terms no longer change the sum (meant for x <= 1)."""
    x = np.asarray(x, np.float64)
    s, term = np.zeros_like(x), np.ones_like(x)
    for n in range(1, 200):
        term = term * (-x / n)
        c = term / n
        s = s + c
        if np.all(np.abs(c) <= 1e-17 * np.abs(s)):
            break
    return -EULER - np.log(x) - s


def e1_cf(x):
    """e^-x / (x+1 - 1/(x+3 - 4/(x+5 - ...))) by the modified Lentz method to 1e-16 (meant for x > 1)."""
    x = np.asarray(x, np.float64)
    b = x + 1.0
    c = np.full_like(x, 1e300)
    d = 1.0 / b
    h = d.copy()
    live = np.ones(x.shape, bool)
    for i in range(1, 201):
        an = -float(i) * i
        b = b + 2.0
        d = 1.0 / (an * d + b)
        c = b + an / c
        de = c * d
        h = np.where(live, h * de, h)
        live = live & ~(np.abs(de - 1.0) < 1e-16)
        if not live.any():
            break
    return h * np.exp(-x)


def e1(x):
    x = np.atleast_1d(np.asarray(x, np.float64))
    out = np.empty_like(x)
    lo = x <= 1.0
    if lo.any():
        out[lo] = e1_series(x[lo])
    if (~lo).any():
        out[~lo] = e1_cf(x[~lo])
    return out


# ---- the recursion
def recursion(Y, **params):
    """The definition's loop on a spectrum Y [T][D].  dict: G [T][D], vad [T], noise [T] (the VAD's decisions), margin =
    min_t |vad_t - eta|, and what the frames exercised: cap (the gamma cap was reached), floor (the xi floor), v_le1 / v_gt1."""
    p = dict(DEFAULTS)
    p.update(params)
    alpha, mu, eta, gmax, init = p["alpha"], p["mu"], p["eta"], p["gamma_max"], int(p["init_frames"])
    xi_min = 10.0 ** (p["xi_min_db"] / 10.0)
    P = Y.real.astype(np.float64) ** 2 + Y.imag.astype(np.float64) ** 2
    T, D = P.shape
    lam = np.maximum(P[:min(init, T)].mean(axis=0), LAMBDA_FLOOR)
    A_prev = np.zeros(D)
    G = np.zeros((T, D))
    vad = np.zeros(T)
    seen = dict(cap=False, floor=False, v_le1=False, v_gt1=False)
    for t in range(T):
        raw = P[t] / lam
        gamma = np.minimum(raw, gmax)
        dd = np.full(D, alpha) if t == 0 else alpha * A_prev / lam
        xi_raw = dd + (1.0 - alpha) * np.maximum(gamma - 1.0, 0.0)
        xi = np.maximum(xi_raw, xi_min)
        vad[t] = np.sum(gamma * xi / (1.0 + xi) - np.log1p(xi)) / D
        A = xi / (1.0 + xi)
        v = A * gamma
        pos = P[t] > 0.0
        g = np.zeros(D)
        if pos.any():
            g[pos] = A[pos] * np.exp(0.5 * e1(v[pos]))
            seen["v_le1"] |= bool((v[pos] <= 1.0).any())
            seen["v_gt1"] |= bool((v[pos] > 1.0).any())
        seen["cap"] |= bool((raw >= gmax).any())
        seen["floor"] |= bool((xi_raw <= xi_min).any())
        if vad[t] < eta:
            lam = np.maximum(mu * lam + (1.0 - mu) * P[t], LAMBDA_FLOOR)
        A_prev = g * g * P[t]
        G[t] = g
    out = dict(G=G, vad=vad, noise=vad < eta, margin=float(np.min(np.abs(vad - eta))))
    out.update(seen)
    return out


def enhance(x, fea_dim, **params):
    """One sentence from PCM: dict of pcm [n], G, vad, noise, margin, ... (recursion) and absY [T][D]."""
    x = np.asarray(x, np.float64)
    Y = analysis(x, fea_dim)
    r = recursion(Y, **params)
    g32 = r["G"].astype(np.float32).astype(np.float64)          # S_t[k] = fl32(G) Y_t[k]
    r["pcm"] = overlap_add(g32 * Y, x.size)
    r["absY"] = np.abs(Y)
    return r


# ---- fixtures
LEAD_HOPS = 7.5          # noise only: the noise start (6 frames) must not swallow the signal


def gated_tones(seed, n, fea_dim, snr_db, sigma=300.0):
    """White noise (std sigma) plus tones gated on and off behind a noise-only lead of 7.5 hops, rounded to int16 values."""
    rng = np.random.default_rng(seed)
    hop = fea_dim - 1
    lead = int(LEAD_HOPS * hop)
    t = np.arange(n)
    noise = rng.normal(0.0, sigma, n)
    sig = np.zeros(n)
    amp = sigma * np.sqrt(2.0 * 10.0 ** (snr_db / 10.0) / 3.0)
    for _ in range(3):
        f = rng.uniform(0.04, 0.42)
        period = int(rng.integers(8, 14)) * hop
        phase = int(rng.integers(0, period))
        gate = ((t + phase) % period) < period // 2
        sig += amp * np.sin(2.0 * np.pi * f * t + rng.uniform(0, 2 * np.pi)) * gate
    sig[:lead] = 0.0
    return np.clip(np.round(noise + sig), -32768, 32767).astype(np.float32)


# (fea_dim, [(kind, samples, seed, snr_db)]): "tones" and "gap" are the sentences that must exercise every branch; the rest are edge cases.
# A sentence whose VAD margin misses 1e-3 gets another seed (tests/test_classic_host.py); the margin does not move.
FIXTURE_SPEC = [
    (33, [("tones", 1500, 1, 5.0), ("tones", 6000, 2, 10.0), ("one", 1, 0, 0.0), ("short", 200, 3, 0.0), ("zero", 1500, 0, 0.0),
          ("gap", 1500, 4, 5.0)]),
    (129, [("tones", 6000, 15, 0.0), ("tones", 9000, 6, 10.0), ("one", 1, 0, 0.0), ("short", 200, 7, 0.0), ("zero", 1500, 0, 0.0),
           ("gap", 6000, 8, 5.0)]),
    (257, [("tones", 9000, 9, 5.0), ("tones", 6000, 10, 0.0), ("one", 1, 0, 0.0), ("short", 200, 11, 0.0), ("zero", 1500, 0, 0.0),
           ("gap", 9000, 12, 10.0)]),
    # (appended: tests index the entries above by position)
    (65, [("tones", 3000, 61, 5.0), ("tones", 6000, 62, 10.0), ("one", 1, 0, 0.0), ("short", 200, 63, 0.0), ("zero", 1500, 0, 0.0),
          ("gap", 3000, 64, 5.0)]),
]


def make_sentence(kind, n, seed, snr_db, fea_dim):
    if kind == "one":
        return np.array([1234.0], np.float32)
    if kind == "zero":
        return np.zeros(n, np.float32)
    if kind == "short":                                          # T < init_frames at fea_dim 65, 129 and 257
        return np.round(np.random.default_rng(seed).normal(0.0, 300.0, n)).astype(np.float32)
    x = gated_tones(seed, n, fea_dim, snr_db)
    if kind == "gap":                                            # an exact-zero stretch of 3.5 hops: whole frames with P = 0
        hop = fea_dim - 1
        a = int(12.25 * hop) if n > 20 * hop else int(9.25 * hop)
        x[a:a + int(3.5 * hop)] = 0.0
    return x


# fea_dim 513 and 1025 (3 and 5 bins per thread on the device): per call a tones sentence that is held to the restatement, one sample,
# and a second tones sentence that is only compared alone against in the batch.  (fea_dim, [(seed, samples, snr_db)])
WIDE_SPEC = [(513, [(553, 14 * 512, 5.0), None, (554, 9 * 512 + 3, 0.0)]), (1025, [(1065, 14 * 1024, 5.0), None, (1066, 9 * 1024 + 3, 0.0)])]


def wide_fixtures():
    """[(fea_dim, sentences)]: sentence 0 is the one the tests hold to the restatement."""
    return [(D, [np.array([7.0], np.float32) if e is None else gated_tones(e[0], e[1], D, e[2]) for e in spec]) for D, spec in WIDE_SPEC]


def fixtures():
    """[(fea_dim, kinds, sentences)], one entry per call of the GPU tests."""
    return [(D, [s[0] for s in spec], [make_sentence(k, n, seed, snr, D) for k, n, seed, snr in spec]) for D, spec in FIXTURE_SPEC]


_REF = {}


def reference(fea_dim, index, **params):
    """enhance() of fixture sentence `index` of the fea_dim call, computed once per parameter set and shared by the tests."""
    key = (fea_dim, index, tuple(sorted(params.items())))
    if key not in _REF:
        for D, _, xs in fixtures():
            if D == fea_dim:
                _REF[key] = enhance(xs[index], fea_dim, **params)
    return _REF[key]


def snr_db(ref, x):
    ref, x = np.asarray(ref, np.float64), np.asarray(x, np.float64)
    return 10.0 * np.log10(np.sum(ref ** 2) / max(np.sum((ref - x) ** 2), 1e-300))
