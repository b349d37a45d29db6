"""NumPy restatement of the MFCC auxiliary target (include/bp_c_api.h), written from the formulas of the
definition, not from the sources: float64 everywhere except where the definition says fp32 (the rounded tables, e, logmel, c,
the target).  The sums that define bits are Python loops of float64 additions in the stated order; a product of two fp32 values
is exact in float64, so each step is one rounded addition.

A `geo` is a dict of fea_dim, sample_rate, n_mel, n_ceps, first_coef, lifter (and optionally f_lo, f_hi: 0 and sample_rate / 2).
The mutants of the definition (MUTANTS) are restated here too: a test shows that each misses its bars by a wide factor."""
import numpy as np

LN_FLOOR32 = np.float32(-23.025850929940457)          # ln(1e-10), the floor of the project's LPS

# fea_dim, sample_rate, n_mel, n_ceps, first_coef, lifter
GEOMETRIES = [
    dict(fea_dim=33, sample_rate=8000, n_mel=8, n_ceps=5, first_coef=1, lifter=0.0),
    dict(fea_dim=129, sample_rate=8000, n_mel=26, n_ceps=13, first_coef=0, lifter=22.0),
    dict(fea_dim=257, sample_rate=16000, n_mel=40, n_ceps=13, first_coef=0, lifter=22.0),
    dict(fea_dim=1025, sample_rate=16000, n_mel=64, n_ceps=20, first_coef=1, lifter=22.0),
    # (appended: tests index the entries above by position)
    dict(fea_dim=65, sample_rate=8000, n_mel=12, n_ceps=8, first_coef=0, lifter=22.0),
    dict(fea_dim=513, sample_rate=16000, n_mel=48, n_ceps=16, first_coef=1, lifter=22.0),
]
MUTANTS = ("edges_shifted", "j_for_j_half", "no_lifter", "log10", "c0_present")


def geo_id(g):
    return "%d-%d-%d-%d-%d-%g" % (g["fea_dim"], g["sample_rate"], g["n_mel"], g["n_ceps"], g["first_coef"], g["lifter"])


def band(g):
    lo = np.float64(np.float32(g.get("f_lo", 0.0)))
    hi = np.float64(np.float32(g.get("f_hi", 0.5 * g["sample_rate"])))
    return lo, hi


def mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_inv(m):
    return 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)


def edges(g):
    """e_p, p = 0 .. n_mel + 1 in Hz: e_0 = f_lo and e_{n_mel+1} = f_hi as given, equally spaced in mel between them."""
    lo, hi = band(g)
    n = g["n_mel"]
    p = np.arange(n + 2, dtype=np.float64)
    e = mel_inv(mel(lo) + (mel(hi) - mel(lo)) * p / (n + 1))
    e[0], e[-1] = lo, hi
    return e


def bin_hz(g):
    M = g["fea_dim"] - 1
    return np.arange(g["fea_dim"], dtype=np.float64) * g["sample_rate"] / (2.0 * M)


def filters64(g, mutant=None):
    """w [n_mel][fea_dim] in float64, before the rounding."""
    e, f = edges(g), bin_hz(g)
    if mutant == "edges_shifted":
        f = f + g["sample_rate"] / (2.0 * (g["fea_dim"] - 1))          # every edge one bin lower
    w = np.zeros((g["n_mel"], g["fea_dim"]))
    for j in range(g["n_mel"]):
        up = (f - e[j]) / (e[j + 1] - e[j])
        down = (e[j + 2] - f) / (e[j + 2] - e[j + 1])
        w[j] = np.maximum(0.0, np.minimum(up, down))
    return w


def filters(g, mutant=None):
    """(w fp32, first_bin, n_bins); ValueError naming the first filter without a bin."""
    w = filters64(g, mutant).astype(np.float32)
    first, nb = np.zeros(g["n_mel"], np.int32), np.zeros(g["n_mel"], np.int32)
    for j in range(g["n_mel"]):
        k = np.nonzero(w[j] > 0)[0]
        if k.size == 0:
            raise ValueError("mel filter %d holds no bin" % j)
        assert np.array_equal(k, np.arange(k[0], k[-1] + 1))
        first[j], nb[j] = k[0], k.size
    return w, first, nb


def dct64(g, mutant=None):
    n, L = g["n_mel"], float(g["lifter"])
    first = 0 if mutant == "c0_present" else g["first_coef"]
    t = np.zeros((g["n_ceps"], n))
    for r in range(g["n_ceps"]):
        i = first + r
        lift = 1.0 + 0.5 * L * np.sin(np.pi * i / L) if L > 0 and mutant != "no_lifter" else 1.0
        j = np.arange(n, dtype=np.float64) + (0.0 if mutant == "j_for_j_half" else 0.5)
        t[r] = lift * np.sqrt(2.0 / n) * np.cos(np.pi * i * j / n)
    return t


def dct(g, mutant=None):
    return dct64(g, mutant).astype(np.float32)


def mel_energy(power, w, first, nb):
    """e [T][n_mel] fp32 from power [T][fea_dim] fp32 and the fp32 table: one float64 accumulator per (frame, filter), bins ascending."""
    power, w = np.asarray(power, np.float32), np.asarray(w, np.float32)
    E = np.zeros((power.shape[0], w.shape[0]), np.float64)
    for j in range(w.shape[0]):
        acc = np.zeros(power.shape[0], np.float64)
        for k in range(int(first[j]), int(first[j]) + int(nb[j])):
            acc = acc + np.float64(w[j, k]) * power[:, k].astype(np.float64)      # (exact product, one rounded addition)
        E[:, j] = acc
    return E.astype(np.float32)


def log_floor(e, mutant=None):
    """logmel in float64 from fp32 e: ln with the 1e-10 floor (the device's fp32 logf is compared with this in ulp)."""
    e = np.asarray(e, np.float32)
    fn = np.log10 if mutant == "log10" else np.log
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(e > np.float32(1e-10), fn(np.maximum(e.astype(np.float64), 1e-300)), np.float64(LN_FLOOR32))


def cepstrum(logmel, t, mean=None, scale=None):
    """target [T][n_ceps] fp32 from fp32 logmel and the fp32 table: one float64 accumulator per (frame, r), filters ascending, then
    fp32: (c - mean) * scale."""
    logmel, t = np.asarray(logmel, np.float32), np.asarray(t, np.float32)
    c = np.zeros((logmel.shape[0], t.shape[0]), np.float32)
    for r in range(t.shape[0]):
        acc = np.zeros(logmel.shape[0], np.float64)
        for j in range(t.shape[1]):
            acc = acc + np.float64(t[r, j]) * logmel[:, j].astype(np.float64)
        c[:, r] = acc.astype(np.float32)
    mean = np.zeros(t.shape[0], np.float32) if mean is None else np.asarray(mean, np.float32)
    scale = np.ones(t.shape[0], np.float32) if scale is None else np.asarray(scale, np.float32)
    return ((c - mean[None, :]).astype(np.float32) * scale[None, :]).astype(np.float32)


def mfcc64(x, g, mutant=None, mean=None, scale=None):
    """The whole chain in float64 from the samples of one sentence (no fp32 step): (e, logmel, target)."""
    import wave_np
    P = np.abs(wave_np.analysis(x, g["fea_dim"])) ** 2
    e = P @ filters64(g, mutant).T
    fn = np.log10 if mutant == "log10" else np.log
    lm = np.where(e > 1e-10, fn(np.maximum(e, 1e-300)), float(LN_FLOOR32))
    c = lm @ dct64(g, mutant).T
    mean = 0.0 if mean is None else np.asarray(mean, np.float64)
    scale = 1.0 if scale is None else np.asarray(scale, np.float64)
    return e, lm, (c - mean) * scale


def ulp_distance(a, ref64):
    """Largest distance of fp32 a from the float64 reference, in units of the fp32 ulp at the reference."""
    a = np.asarray(a, np.float32)
    r32 = np.asarray(ref64, np.float64).astype(np.float32)
    ulp = np.spacing(np.abs(r32)).astype(np.float64)
    return float(np.max(np.abs(a.astype(np.float64) - np.asarray(ref64, np.float64)) / ulp)) if a.size else 0.0


def sentence_lengths(g, rng):
    """Lengths 1, hop - 1, n_fft - 1, four random ones up to 6 n_fft; the silent sentence of 3 hop comes last."""
    hop = g["fea_dim"] - 1
    n_fft = 2 * hop
    return [1, hop - 1, n_fft - 1] + [int(v) for v in rng.integers(1, 6 * n_fft + 1, size=4)] + [3 * hop]


def make_sentences(g, seed):
    rng = np.random.default_rng(seed)
    lens = sentence_lengths(g, rng)
    sents = [(rng.normal(size=n) * 3000.0).astype(np.float32) for n in lens[:-1]]
    sents.append(np.zeros(lens[-1], np.float32))
    return sents
