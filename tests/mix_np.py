"""NumPy restatement of the training mixtures of bp_set_mix_corpus / bp_train_mix (include/bp_c_api.h): the
plan and the shuffles (Philox4x32-10 of tests/philox_np.py), the gain, the mixed samples, the clean and noise spectra, the targets
and the noise-aware rows, in float64 where the definition does not name a float32 step.  Written from the definition, not from
csrc/bp_mix.hip; the analysis is tests/wave_np.py."""
import numpy as np

import philox_np as PX
import wave_np as WN

LPS, IRM, IBM, LPS_IRM, LPS_IBM = 0, 1, 2, 3, 4


def _philox(seed, c0, c1, c2, c3=0):
    w = PX.philox4x32_10(np.array([c0], np.uint64), np.array([c1], np.uint64), np.array([c2], np.uint64), np.array([c3], np.uint64),
                         seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [int(x[0]) for x in w]


def _scale(u, n):
    return (int(u) * int(n)) >> 32


def plan(seed, n_clean, per_clean, noise_lens, snr_list):
    """list of (clean, noise, offset, snr_db) tuples, snr_db as float32."""
    out = []
    for m in range(n_clean * per_clean):
        u = _philox(seed, m, 0, 0)
        k = _scale(u[0], len(noise_lens))
        out.append((m // per_clean, k, _scale(u[1], noise_lens[k]), np.float32(snr_list[_scale(u[2], len(snr_list))])))
    for i in range(len(out) - 1, 0, -1):
        j = _scale(_philox(seed, i, 0, 1)[0], i + 1)
        out[i], out[j] = out[j], out[i]
    return out


def shuffle(seed, stream, n):
    a = list(range(n))
    for i in range(n - 1, 0, -1):
        j = _scale(_philox(seed, i, stream, 2)[0], i + 1)
        a[i], a[j] = a[j], a[i]
    return np.array(a, np.int64)


def segment(noise, offset, n):
    """v[i] = noise[(offset + i) mod len], i < n."""
    return np.asarray(noise, np.float32)[(offset + np.arange(n)) % len(noise)]


def gain(s, v, snr_db):
    """float32 gain: sqrt(E_s / (E_v 10^(snr/10))) in float64, rounded once; 0 for silent noise."""
    Es = float(np.sum(np.asarray(s, np.float64) ** 2))
    Ev = float(np.sum(np.asarray(v, np.float64) ** 2))
    return np.float32(0.0) if Ev == 0 else np.float32(np.sqrt(Es / (Ev * 10.0 ** (float(snr_db) / 10.0))))


def mixture(clean, noise, mix):
    """x (float64 of g v + s), the clean samples, the float32 products g v and g, for one mixture (c, n, o, snr)."""
    c, n, o, snr = mix
    s = np.asarray(clean[c], np.float32)
    v = segment(noise[n], o, s.size)
    g = gain(s, v, snr)
    gv = (g * v).astype(np.float32)
    return np.float64(g) * v.astype(np.float64) + s, s, gv, g


def targets(S, N, target, lc_db):
    """Target rows [T][fea_dim or 2 fea_dim] from the clean and noise spectra."""
    ps, pn = np.abs(S) ** 2, np.abs(N) ** 2
    lps = np.log(np.maximum(ps, 1e-10))
    irm = np.sqrt(ps / np.maximum(ps + pn, 1e-10))
    ibm = (ps > 10.0 ** (lc_db / 10.0) * pn).astype(np.float64)
    return {LPS: lps, IRM: irm, IBM: ibm, LPS_IRM: np.concatenate([lps, irm], 1), LPS_IBM: np.concatenate([lps, ibm], 1)}[target]


def ibm_margin(S, N, lc_db):
    """|ratio / threshold - 1| per bin (the IBM decisions close to the threshold), inf where the noise bin is 0."""
    ps, pn = np.abs(S) ** 2, np.abs(N) ** 2
    thr = 10.0 ** (lc_db / 10.0) * pn
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(thr > 0, np.abs(ps / np.where(thr > 0, thr, 1.0) - 1.0), np.inf)


def features(clean, noise, plan_, fea_dim, mean, inv_std, target, lc_db):
    """Per mixture: x, S, N (spectra of s and g v), Y (of x), normalised noisy frames z, targets and the NAT row."""
    out = []
    for mix in plan_:
        x, s, gv, g = mixture(clean, noise, mix)
        S, N, Y = WN.analysis(s, fea_dim), WN.analysis(gv, fea_dim), WN.analysis(x, fea_dim)
        z = (WN.lps(Y) - mean) * inv_std
        out.append(dict(x=x, g=g, S=S, N=N, Y=Y, z=z, targ=targets(S, N, target, lc_db), nat=WN.nat_row(z)))
    return out


def window_tables(frames, context, order=None):
    """Host-built window tables of a call per the definition: staged row of mixture-frame g = g + m (context-1) + ..., so
    win_start[i] = order[i] + m(order[i]) (context - 1), targ_frame[i] = order[i], nat_row[i] = m(order[i])."""
    frames = np.asarray(frames, np.int64)
    F = np.concatenate([[0], np.cumsum(frames)])
    n = int(F[-1])
    order = np.arange(n) if order is None else np.asarray(order, np.int64)
    m = np.searchsorted(F, order, side="right") - 1
    return (order + m * (context - 1)).astype(np.int32), order.astype(np.int32), m.astype(np.int32)


def staged_rows(fea, frames, context, targ_offset):
    """The staged raw frames of a chunk from the normalised rows [sum T][D]: mixture m's rows with its first frame repeated
    targ_offset times in front and its last frame context-1-targ_offset times behind."""
    out, f0 = [], 0
    for T in frames:
        z = fea[f0:f0 + T]
        out += [z[:1]] * targ_offset + [z] + [z[-1:]] * (context - 1 - targ_offset)
        f0 += T
    return np.ascontiguousarray(np.concatenate(out).astype(np.float32))
