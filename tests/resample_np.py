"""NumPy restatement of the rational sample-rate converter (bp_resample_*, include/bp_c_api.h), in float64 and
written from the definition in the header, not from the kernel:

  rate_out / rate_in = p / q in lowest terms; m = max(p, q), Lh = zeros m
  g[j] = I0(beta sqrt(1 - ((j - Lh) / Lh)^2)) / I0(beta) * sinc(rolloff (j - Lh) / m),  j = 0 .. 2 Lh
  h[j] = fl32(p g[j] / sum g)
  y[k] = fl32(sum_j h[j] x[(k q + Lh - j) / p]) over the j with p | (k q + Lh - j) and the sample in [0, n), j ascending

The sum is taken one term after the other in ascending j (np.sum is pairwise and is not the definition); only k is vectorised.
An output sample k meets the taps j = r_k, r_k + p, r_k + 2p, ... with r_k = (k q + Lh) mod p, so the i-th pass of the loop adds,
for every k at once, its i-th tap in ascending order.
"""
import math

import numpy as np

DEFAULTS = (16, 8.6, 0.9)


def ratio(rate_in, rate_out):
    """(p, q), or None where the header says BP_ERR_ARG."""
    if rate_in < 1 or rate_out < 1:
        return None
    g = math.gcd(rate_in, rate_out)
    p, q = rate_out // g, rate_in // g
    return (p, q) if max(p, q) <= 1024 else None


def length(n, p, q):
    return -((-n * p) // q)


def taps_np(p, q, zeros=16, beta=8.6, rolloff=0.9):
    """The formula with numpy's own kaiser and sinc, float64 (what bp_resample_taps is compared with, not what feeds the kernel's check)."""
    m = max(p, q)
    Lh = zeros * m
    j = np.arange(2 * Lh + 1, dtype=np.float64)
    g = np.kaiser(2 * Lh + 1, beta) * np.sinc(rolloff * (j - Lh) / m)
    return p * g / g.sum()


def resample(x, p, q, h):
    """y of the definition for one sentence x (float32) and taps h (float32, 2 Lh + 1 of them); float32."""
    x = np.asarray(x, np.float32).astype(np.float64)
    h = np.asarray(h, np.float32).astype(np.float64)
    n, Lh = x.size, (h.size - 1) // 2
    k = np.arange(length(n, p, q), dtype=np.int64)
    t0 = k * q + Lh
    r = t0 % p
    acc = np.zeros(k.size, np.float64)
    for i in range((2 * Lh) // p + 1):
        j = r + i * p
        s = (t0 - j) // p                          # exact: p | t0 - j
        ok = (j <= 2 * Lh) & (s >= 0) & (s < n)
        if ok.any():
            acc[ok] = acc[ok] + h[j[ok]] * x[s[ok]]
    return acc.astype(np.float32)


def abs_terms(x, p, q, h):
    """sum_j |h[j] x[...]| per output sample (float64): the scale of the rounding-error bounds."""
    x = np.abs(np.asarray(x, np.float64))
    h = np.abs(np.asarray(h, np.float64))
    n, Lh = x.size, (h.size - 1) // 2
    k = np.arange(length(n, p, q), dtype=np.int64)
    t0 = k * q + Lh
    r = t0 % p
    acc = np.zeros(k.size, np.float64)
    for i in range((2 * Lh) // p + 1):
        j = r + i * p
        s = (t0 - j) // p
        ok = (j <= 2 * Lh) & (s >= 0) & (s < n)
        acc[ok] += h[j[ok]] * x[s[ok]]
    return acc
