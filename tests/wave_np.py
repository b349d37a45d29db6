"""NumPy restatement of the signal layer of bp_enhance_waves / bp_wave_lps (include/bp_c_api.h), in
float64: analysis, normalisation, window stacking with replicated edge frames, the noise-aware block, the forward with CV
semantics, resynthesis and least-squares overlap-add.  Written from the definition, not from csrc/bp_wave.hip."""
import numpy as np

LN_FLOOR = np.log(1e-10)


def geometry(fea_dim):
    n_fft = 2 * (fea_dim - 1)
    return n_fft, n_fft // 2


def n_frames(n, fea_dim):
    n_fft, hop = geometry(fea_dim)
    return (n - 1) // hop + n_fft // hop


def window(n_fft):
    return 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)


def analysis(x, fea_dim):
    """Noisy complex spectrum Y [T][fea_dim] of one sentence."""
    n_fft, hop = geometry(fea_dim)
    x = np.asarray(x, np.float64)
    T = n_frames(x.size, fea_dim)
    P = n_fft - hop
    xp = np.zeros((T - 1) * hop + n_fft)
    xp[P:P + x.size] = x
    fr = np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)]) * window(n_fft)
    return np.fft.rfft(fr, axis=1)


def lps(Y):
    return np.log(np.maximum(np.abs(Y) ** 2, 1e-10))


def nat_row(z):
    """Mean of the first 6 normalised frames, frame index clamped to the sentence (PfileReader::try_nat_rows)."""
    nf = min(6, z.shape[0])
    return sum(z[min(f, nf - 1)] for f in range(6)) / 6.0


def stack(z, context, targ_offset, nat):
    """Network inputs of every frame: frames clamp(t - targ_offset + j, 0, T-1), j < context [+ the NAT row]."""
    T = z.shape[0]
    idx = np.clip(np.arange(T)[:, None] - targ_offset + np.arange(context)[None, :], 0, T - 1)
    x = z[idx].reshape(T, -1)
    if nat:
        x = np.concatenate([x, np.repeat(nat_row(z)[None, :], T, axis=0)], axis=1)
    return x


def forward(W, b, x, activation=0, keep=(1.0, 1.0), out_act=0, out_lin=0):
    """CV-semantics forward: weight layer 1 scaled by keep[0], the others by keep[1] (dropoutflag), ReLU / sigmoid hidden
    units, linear output or logistic on the columns from out_lin on."""
    L = len(W)
    h = np.asarray(x, np.float64)
    for l in range(1, L):
        z = (keep[0] if l == 1 else keep[1]) * (h @ np.asarray(W[l], np.float64)) + np.asarray(b[l], np.float64)
        if l < L - 1:
            h = np.maximum(z, 0.0) if activation == 0 else 1.0 / (1.0 + np.exp(-z))
        else:
            h = z.copy()
            if out_act == 1:
                h[:, out_lin:] = 1.0 / (1.0 + np.exp(-z[:, out_lin:]))
    return h


def resynth(Y, o, target, n):
    """S from the net columns o [T][fea_dim] and Y, then sum_t w irfft(S_t) / sum_t w^2, trimmed to n samples."""
    T, D = Y.shape
    n_fft, hop = geometry(D)
    o = np.asarray(o, np.float64)
    if target == 0:
        mag = np.abs(Y)
        ph = np.where(mag > 0, Y / np.where(mag > 0, mag, 1.0), 1.0)
        S = np.exp(o / 2) * ph
    else:
        S = o * Y
    w = window(n_fft)
    fr = np.fft.irfft(S, n=n_fft, axis=1) * w
    num = np.zeros((T - 1) * hop + n_fft)
    den = np.zeros_like(num)
    for t in range(T):
        num[t * hop:t * hop + n_fft] += fr[t]
        den[t * hop:t * hop + n_fft] += w * w
    P = n_fft - hop
    return (num / np.where(den > 0, den, 1.0))[P:P + n]


def norm_stats(sentences, fea_dim):
    """Per-bin mean and inverse standard deviation over all frames of the sentences (bpfeat norm_out)."""
    L = np.concatenate([lps(analysis(x, fea_dim)) for x in sentences])
    return L.mean(0), 1.0 / L.std(0)


def identity_net(fea_dim, context, targ_offset, nat, mean, inv_std):
    """Three layers that reproduce the LPS of the centre frame: hidden k = ReLU(z_k), D+k = ReLU(-z_k), out = (h_k - h_{D+k})
    / inv_std_k + mean_k.  The NAT block (when present) gets zero weights."""
    D = fea_dim
    s0 = (context + (1 if nat else 0)) * D
    W1 = np.zeros((s0, 2 * D), np.float32)
    for k in range(D):
        W1[targ_offset * D + k, k] = 1.0
        W1[targ_offset * D + k, D + k] = -1.0
    W2 = np.zeros((2 * D, D), np.float32)
    for k in range(D):
        W2[k, k] = 1.0 / inv_std[k]
        W2[D + k, k] = -1.0 / inv_std[k]
    return [s0, 2 * D, D], [None, W1, W2], [None, np.zeros(2 * D, np.float32), np.asarray(mean, np.float32).copy()]


def make_sentences(rng, lengths, scale=3000.0):
    """PCM16-like sentences (integers in int16 range)."""
    return [np.clip(np.round(rng.normal(0.0, scale, size=n)), -32768, 32767).astype(np.float32) for n in lengths]
