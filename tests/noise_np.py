"""NumPy restatement of the log-MMSE baseline with the MMSE-SPP noise tracker (bp_logmmse_waves_nt, include/bp_c_api.h,
INTEGRATION.md 1n), in float64 and from the PCM samples on.  Written from the definition; it calls nothing in the library.  The
signal layer, the exponential integral and the overlap-add are classic_np's; the recursion is restated here because the tracker's
update sits in front of the frame's gain.  Also the fixture sentences of tests/test_noise_host.py and tests/test_noise_gpu.py, and
the mutants the host test shows to miss the bar."""
import numpy as np

import classic_np as CN

NOISE_DEFAULTS = dict(mode=1, xi_h1_db=15.0, q=0.5, a_pow=0.8, a_spp=0.9, p_lo=0.98, p_cap=0.99)
MODE_VAD, MODE_SPP = 0, 1
MUTANTS = ("no_ceiling", "hard_ceiling", "update_behind", "pbar_carried", "a_swapped", "no_c1")
# A parameter set under which pbar climbs into the ramp in EVERY bin within a dozen frames of noise (at the defaults only the bins
# of a sustained tone get there, after some 40 frames): the state a stream carries between pushes then moves every bin's lambda.
BUSY = dict(q=0.9, xi_h1_db=0.0, a_spp=0.7, p_lo=0.4, p_cap=0.8)


def constants(noise):
    xi = 10.0 ** (noise["xi_h1_db"] / 10.0)
    return (1.0 - noise["q"]) / noise["q"] * (1.0 + xi), xi / (1.0 + xi)


def recursion(Y, lm=None, noise=None, mutant=None, pbar0=None):
    """The definition's loop on a spectrum Y [T][D].  dict: G [T][D], vad [T], noise [T][D] (the lambda frame t's gamma used, in
    either mode), pbar [D] at the end, and in tracker mode ramp / full: the frame-bins with 0 < r < 1 and with r == 1."""
    p = dict(CN.DEFAULTS)
    p.update(lm or {})
    n = dict(NOISE_DEFAULTS)
    n.update(noise or {})
    alpha, mu, eta, gmax, init = p["alpha"], p["mu"], p["eta"], p["gamma_max"], int(p["init_frames"])
    xi_min = 10.0 ** (p["xi_min_db"] / 10.0)
    spp = int(n["mode"]) == MODE_SPP
    a_pow, a_spp, p_lo, p_cap = n["a_pow"], n["a_spp"], n["p_lo"], n["p_cap"]
    if mutant == "a_swapped":
        a_pow, a_spp = a_spp, a_pow
    c0, c1 = constants(n)
    if mutant == "no_c1":
        c1 = 1.0
    P = Y.real.astype(np.float64) ** 2 + Y.imag.astype(np.float64) ** 2
    T, D = P.shape
    lam = np.maximum(P[:min(init, T)].mean(axis=0), CN.LAMBDA_FLOOR)
    pbar = np.zeros(D) if pbar0 is None else np.array(pbar0, np.float64)
    A_prev = np.zeros(D)
    G, vad, N = np.zeros((T, D)), np.zeros(T), np.zeros((T, D))
    ramp = full = 0

    def track(lam, pbar):
        nonlocal ramp, full
        ph = 1.0 / (1.0 + c0 * np.exp(-c1 * P[t] / lam))
        pbar = a_spp * pbar + (1.0 - a_spp) * ph
        r = np.clip((pbar - p_lo) / (p_cap - p_lo), 0.0, 1.0)
        if mutant == "hard_ceiling":
            r = (pbar > p_cap).astype(np.float64)
        if mutant == "no_ceiling":
            r = np.zeros(D)
        ramp += int(((r > 0.0) & (r < 1.0)).sum())
        full += int((r == 1.0).sum())
        ph = np.minimum(ph, 1.0 - (1.0 - p_cap) * r)
        lam = np.maximum(a_pow * lam + (1.0 - a_pow) * ((1.0 - ph) * P[t] + ph * lam), CN.LAMBDA_FLOOR)
        return lam, pbar

    for t in range(T):
        if spp and mutant != "update_behind":
            lam, pbar = track(lam, pbar)
        N[t] = lam
        gamma = np.minimum(P[t] / lam, gmax)
        dd = np.full(D, alpha) if t == 0 else alpha * A_prev / lam
        xi = np.maximum(dd + (1.0 - alpha) * np.maximum(gamma - 1.0, 0.0), xi_min)
        vad[t] = np.sum(gamma * xi / (1.0 + xi) - np.log1p(xi)) / D
        A = xi / (1.0 + xi)
        v = A * gamma
        pos = P[t] > 0.0
        g = np.zeros(D)
        if pos.any():
            g[pos] = A[pos] * np.exp(0.5 * CN.e1(v[pos]))
        if spp and mutant == "update_behind":
            lam, pbar = track(lam, pbar)
        if not spp and vad[t] < eta:
            lam = np.maximum(mu * lam + (1.0 - mu) * P[t], CN.LAMBDA_FLOOR)
        A_prev = g * g * P[t]
        G[t] = g
    return dict(G=G, vad=vad, noise=N, pbar=pbar, ramp=ramp, full=full)


def enhance(x, fea_dim, lm=None, noise=None, mutant=None, pbar0=None):
    """One sentence from PCM: recursion() plus pcm [n] and absY [T][D]."""
    x = np.asarray(x, np.float64)
    Y = CN.analysis(x, fea_dim)
    r = recursion(Y, lm, noise, mutant, pbar0)
    g32 = r["G"].astype(np.float32).astype(np.float64)
    r["pcm"] = CN.overlap_add(g32 * Y, x.size)
    r["absY"] = np.abs(Y)
    return r


# ---- fixtures
SIGMA = 300.0
SUSTAINED_FRAMES, STEP_FRAMES = 62, 120
STEP_SIGMA = (100.0, 200.0)
SEEDS = {33: (331, 332), 65: (651, 652), 129: (1291, 1292), 257: (2571, 2572)}     # (sustained, step)


def sustained(seed, fea_dim):
    """White noise (sigma 300) and, from hop 7.5 to the end of 62 frames, two steady tones of amplitude 6 sigma."""
    rng = np.random.default_rng(seed)
    hop = fea_dim - 1
    n = (SUSTAINED_FRAMES - 2) * hop + 1
    t = np.arange(n)
    x = rng.normal(0.0, SIGMA, n)
    sig = np.zeros(n)
    for _ in range(2):
        f = rng.uniform(0.06, 0.40)
        sig += 6.0 * SIGMA * np.sin(2.0 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    sig[:int(CN.LEAD_HOPS * hop)] = 0.0
    return np.clip(np.round(x + sig), -32768, 32767).astype(np.float32)


def step(seed, fea_dim):
    """White noise whose sigma goes from 100 to 200 at the middle of 120 frames."""
    rng = np.random.default_rng(seed)
    hop = fea_dim - 1
    n = (STEP_FRAMES - 2) * hop + 1
    x = rng.normal(0.0, 1.0, n)
    x[:n // 2] *= STEP_SIGMA[0]
    x[n // 2:] *= STEP_SIGMA[1]
    return np.round(x).astype(np.float32)


def ceiling_share(x, fea_dim, noise):
    """(ramp, full, share): the frame-bins inside the ramp and at the full ceiling, and the share of the bins whose lambda the
    ceiling -- and so the carried pbar -- moves by more than 1e-3 somewhere in the sentence."""
    Y = CN.analysis(np.asarray(x, np.float64), fea_dim)
    r, m = recursion(Y, None, noise), recursion(Y, None, noise, mutant="no_ceiling")
    moved = (np.abs(r["noise"] - m["noise"]) / r["noise"]).max(axis=0) > 1e-3
    return r["ramp"], r["full"], float(moved.mean())


def step_level_db(noise_rows, fea_dim):
    """Mean of noise_t over frames T-12 .. T-3 and all bins, in dB relative to the true noise power sigma_end^2 sum w^2."""
    T = noise_rows.shape[0]
    true = STEP_SIGMA[1] ** 2 * np.sum(CN.window(2 * (fea_dim - 1)) ** 2)
    return 10.0 * np.log10(np.mean(np.asarray(noise_rows, np.float64)[T - 12:T - 2]) / true)


_FIX = {}


def fixtures():
    """[(fea_dim, kinds, sentences)], one entry per call of the GPU tests: classic_np's sentences, then sustained and step.  (The
    longest of this file's own sentences has 120 frames; classic_np's 6000 samples at fea_dim 33 have 189.)"""
    if not _FIX:
        out = []
        for D, kinds, xs in CN.fixtures():
            a, b = SEEDS[D]
            out.append((D, list(kinds) + ["sustained", "step"], list(xs) + [sustained(a, D), step(b, D)]))
        _FIX["f"] = sorted(out, key=lambda e: e[0])
    return _FIX["f"]


def fixture(fea_dim):
    return [f for f in fixtures() if f[0] == fea_dim][0]


def wide_fixtures():
    """[(fea_dim, [one tones sentence])] at 513 and 1025."""
    return [(D, [xs[0]]) for D, xs in CN.wide_fixtures()]


_REF = {}


def reference(fea_dim, index, mode=MODE_SPP):
    """enhance() of fixture sentence `index` of the fea_dim call at the defaults, computed once and shared by the tests."""
    key = (fea_dim, index, mode)
    if key not in _REF:
        xs = fixture(fea_dim)[2] if fea_dim <= 257 else [w for w in wide_fixtures() if w[0] == fea_dim][0][1]
        _REF[key] = enhance(xs[index], fea_dim, noise=dict(mode=mode))
    return _REF[key]
