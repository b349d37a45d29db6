"""Why one bar of 1e-5 holds the signal layer at every frame size: the restatement of tests/wave_np.py run in float32 against
itself in float64, on the sentences of tests/geometry_cases.py.  Derived from the reference alone, on the CPU: torch.fft on
float32 frames, float32 window, float32 overlap-add; the net outputs are the float64 forward of the cases' own net, rounded once
and given to both sides (as the GPU tests give the device's out_net to the restatement).

Measured (python tests/test_wave_f32_host.py prints the table): analysis 5.0e-7 .. 5.3e-7 (half an ulp of an LPS value near 20,
which the float32 feature carries), resynthesis 1.3e-7 .. 3.2e-7, the all-zero frames against their own segment 2.6e-7 .. 8.0e-7;
no growth towards 1025.  The project's 1e-5 therefore leaves more than 12 x over an fp32 implementation at all six sizes and a
size-dependent bar is not justified.  The test holds every figure to 1e-6: a tenth of the bar."""
import numpy as np
import pytest
import torch

import geometry_cases as GC
import wave_np as WN

F32_BAR = 1e-6


def analysis32(x, fea_dim):
    n_fft, hop = WN.geometry(fea_dim)
    T = WN.n_frames(x.size, fea_dim)
    xp = np.zeros((T - 1) * hop + n_fft, np.float32)
    xp[n_fft - hop:n_fft - hop + x.size] = x
    fr = np.stack([xp[t * hop:t * hop + n_fft] for t in range(T)]) * WN.window(n_fft).astype(np.float32)
    return torch.fft.rfft(torch.from_numpy(fr), dim=1).numpy()


def resynth32(Y, o, target, n):
    T, D = Y.shape
    n_fft, hop = WN.geometry(D)
    o = np.asarray(o, np.float32)
    if target == 0:
        mag = np.abs(Y)
        ph = np.where(mag > 0, Y / np.where(mag > 0, mag, np.float32(1.0)), np.complex64(1.0))
        S = (np.exp(o * np.float32(0.5)) * ph).astype(np.complex64)
    else:
        S = (o * Y).astype(np.complex64)
    w = WN.window(n_fft).astype(np.float32)
    fr = torch.fft.irfft(torch.from_numpy(S), n=n_fft, dim=1).numpy() * w
    num = np.zeros((T - 1) * hop + n_fft, np.float32)
    den = np.zeros_like(num)
    for t in range(T):
        num[t * hop:t * hop + n_fft] += fr[t]
        den[t * hop:t * hop + n_fft] += w * w
    assert num.dtype == np.float32 and fr.dtype == np.float32
    return (num / np.where(den > 0, den, np.float32(1.0)))[n_fft - hop:n_fft - hop + n]


def net_outputs(fea_dim, target, xs):
    """The cases' net on the float64 features, per sentence [T][D] float32: LPS columns, or the logistic mask block."""
    from oracle import bp_numpy as N
    ls = GC.net_sizes(fea_dim, target)
    W, b = N.glorot_net(ls, seed=5, beta=0.5)
    m, i = WN.norm_stats(xs, fea_dim)
    out = []
    for x in xs:
        z = (WN.lps(WN.analysis(x, fea_dim)) - m) * i
        o = WN.forward(W, b, WN.stack(z, GC.CTX, GC.TOFF, True), out_act=int(target == "mask"), out_lin=fea_dim)
        out.append(o[:, -fea_dim:].astype(np.float32))
    return out


def figures(fea_dim):
    """dict(analysis, mask, lps, lps_zero_frames): the float32 restatement's worst error against float64, each as the GPU tests
    measure it (analysis: of the frame's largest magnitude; resynthesis: of the sentence's, or the segment's, largest sample)."""
    xs = GC.sentences(fea_dim)
    Y64 = [WN.analysis(x, fea_dim) for x in xs]
    Y32 = [analysis32(x, fea_dim) for x in xs]
    out = dict(analysis=0.0, mask=0.0, lps=0.0, lps_zero_frames=0.0)
    for a, b in zip(Y32, Y64):
        assert a.dtype == np.complex64
        mag = np.abs(b)
        l = np.log(np.maximum(np.abs(a).astype(np.float32) ** 2, np.float32(1e-10)))
        for t in np.flatnonzero(mag.max(1) > 0):
            out["analysis"] = max(out["analysis"], float(np.abs(np.exp(l[t].astype(np.float64) / 2) - mag[t]).max() / mag[t].max()))
    for target in ("mask", "lps"):
        code = 0 if target == "lps" else 1
        for x, a, b, o in zip(xs, Y32, Y64, net_outputs(fea_dim, target, xs)):
            got, ref = resynth32(a, o, code, x.size), WN.resynth(b, o, code, x.size)
            out[target] = max(out[target], float(np.abs(got - ref).max() / np.abs(ref).max()))
        if target == "lps":
            lo, hi = GC.zero_segment(fea_dim, GC.zero_frames(Y64[-1]))
            assert np.abs(ref[lo:hi]).max() > 0
            out["lps_zero_frames"] = float(np.abs(got - ref)[lo:hi].max() / np.abs(ref[lo:hi]).max())
    return out


@pytest.mark.parametrize("D", GC.FEA_DIMS)
def test_float32_restatement_is_far_below_the_bar(D):
    f = figures(D)
    print("fea_dim %d: %s" % (D, f))
    assert max(f.values()) <= F32_BAR, (D, f)
    assert 10 * F32_BAR <= GC.WAVE_BAR


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("| `fea_dim` | analysis | mask resynthesis | LPS resynthesis | LPS, all-zero frames |\n|---|---|---|---|---|")
    for D in GC.FEA_DIMS:
        f = figures(D)
        print("| %d | %.1e | %.1e | %.1e | %.1e |" % (D, f["analysis"], f["mask"], f["lps"], f["lps_zero_frames"]))
