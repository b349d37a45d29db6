"""NumPy restatement of the dynamic noise-aware input (bp_set_nat, include/bp_c_api.h), in float64: one
noise-aware row per frame, the noise PSD of the MMSE-SPP tracker as a normalised LPS row.  Written from the definition; it calls
nothing in the library.  The tracker is noise_np.recursion's (its `noise` rows are the lambda that frame t's gamma used, which is
the lambda of the definition), the signal layer is wave_np's.  Also the case table of tests/test_dnat_host.py and
tests/test_dnat_gpu.py, the wrong stagings the host test shows to miss the bar, and a net that returns the staged block."""
import numpy as np

import noise_np as NN
import wave_np as WN

MODES = ("static", "dynamic")
FLOOR = 1e-10
MUTANTS = ("static_broadcast", "previous_frame", "sentence_index", "no_mean", "start_over_all_frames")


def lambdas(Y, noise=None, init_frames=6):
    """The tracked noise PSD [T][D] of one sentence's spectrum Y: noise start over min(6, T) frames, then the tracker's step in
    front of every frame."""
    n = dict(NN.NOISE_DEFAULTS)
    n.update(noise or {})
    return NN.recursion(Y, dict(init_frames=init_frames), n)["noise"]


def normalise(lam, mean, inv_std):
    return (np.log(np.maximum(lam, FLOOR)) - np.asarray(mean, np.float64)) * np.asarray(inv_std, np.float64)


def rows(Y, mean, inv_std, noise=None):
    """nat [T][D] of one sentence."""
    return normalise(lambdas(Y, noise), mean, inv_std)


def denormalise(nat, mean, inv_std):
    """log(lambda) from rows the device returned (float64 arithmetic on its fp32 values)."""
    return np.asarray(nat, np.float64) / np.asarray(inv_std, np.float64) + np.asarray(mean, np.float64)


def batch(sentences, fea_dim, mean, inv_std, noise=None):
    """(nat [sum T][D], nat_row [sum T]) of a call: the rows of the sentences one behind the other, and every frame's own index."""
    r = np.concatenate([rows(WN.analysis(x, fea_dim), mean, inv_std, noise) for x in sentences])
    return r, np.arange(r.shape[0])


def blocks(sentences, fea_dim, mean, inv_std, mutant=None):
    """The noise-aware block [sum T][D] that every frame of a call meets: nat[nat_row[g]].  mutant: one of the wrong stagings."""
    Ys = [WN.analysis(x, fea_dim) for x in sentences]
    out = []
    F = 0
    good, _ = batch(sentences, fea_dim, mean, inv_std)
    for s, Y in enumerate(Ys):
        T = Y.shape[0]
        r = rows(Y, mean, inv_std)
        if mutant == "static_broadcast":
            z = (WN.lps(Y) - mean) * inv_std
            r = np.repeat(WN.nat_row(z)[None, :], T, axis=0)
        elif mutant == "previous_frame":
            r = r[np.maximum(np.arange(T) - 1, 0)]
        elif mutant == "sentence_index":
            r = np.repeat(good[s][None, :], T, axis=0)          # nat_row[g] = s: row s of the call's table
        elif mutant == "no_mean":
            r = np.log(np.maximum(lambdas(Y), FLOOR)) * inv_std
        elif mutant == "start_over_all_frames":
            r = normalise(lambdas(Y, init_frames=T), mean, inv_std)
        else:
            assert mutant is None
        out.append(r)
        F += T
    return np.concatenate(out)


def selector_net(fea_dim, context, mean, inv_std):
    """wave_np.identity_net pointed at the LAST fea_dim inputs, the noise-aware block: hidden k = ReLU(nat_k), D+k = ReLU(-nat_k),
    out = (h_k - h_{D+k}) / inv_std_k + mean_k -- the de-normalised block, read back through the forward."""
    D = fea_dim
    ls, W, b = WN.identity_net(D, context, 0, True, mean, inv_std)
    W[1][:] = 0.0
    for k in range(D):
        W[1][context * D + k, k] = 1.0
        W[1][context * D + k, D + k] = -1.0
    return ls, W, b


# ---- the case table: every entry point that stages the block, in both modes, at the sizes at which the kernel can go wrong.
# T classes: the shortest sentence there is (1 sample: 2 frames -- T = (n - 1) / hop + 2 has no 1), fewer frames than the noise
# start, exactly 6, one more, and about 40.  All of them ride in one batch of every case.
ENTRIES = ("enhance_waves", "mix_features", "train_mix", "cv_mix", "eval_mix")
FEA_DIMS = (33, 129)
T_CLASSES = (2, 3, 6, 7, 40)
WIDE = 257                                           # once: the partial last 64-thread workgroup (257 = 4 * 64 + 1)
CONTEXTS = ((3, 1), (1, 0))                          # (context, targ_offset)
# The sizes the frame-size table (tests/geometry_cases.py) adds, at context 3 / targ_offset 1: ceil(D / 64) = 2 (the second
# workgroup with one live thread), 9 and 17 workgroups of 64 threads per sentence or job, next to the 1, 3 and 5 above.
GEOMETRY = (65, 513, 1025)
ALL_DIMS = tuple(sorted(FEA_DIMS + (WIDE,) + GEOMETRY))


def lengths(fea_dim):
    """Sample counts with T_CLASSES frames."""
    hop = fea_dim - 1
    out = [1 if T == 2 else (T - 2) * hop + 1 + (hop // 3 if T > 3 else 0) for T in T_CLASSES]
    assert [WN.n_frames(n, fea_dim) for n in out] == list(T_CLASSES)
    return out


def cases():
    return [dict(mode=m, entry=e, fea_dim=D, T=T) for m in MODES for e in ENTRIES for D in FEA_DIMS for T in T_CLASSES]


def sentences(seed, fea_dim):
    """One sentence per T class: white noise whose level steps up 6 dB in the middle (the tracker has something to follow)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths(fea_dim):
        x = rng.normal(0.0, 300.0, n)
        x[n // 2:] *= 2.0
        out.append(np.clip(np.round(x), -32768, 32767).astype(np.float32))
    return out


def norm(fea_dim, seed=11):
    rng = np.random.default_rng(seed)
    return rng.normal(10.0, 2.0, fea_dim).astype(np.float32), rng.uniform(0.2, 0.5, fea_dim).astype(np.float32)
