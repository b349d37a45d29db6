"""NumPy restatement of the reverberant corpus entries (include/bp_c_api.h): the delay of a room impulse
response, the reverberant sentence r and its direct-plus-early part e, and the pairing of sentences with responses.  Written from
the definition, not from csrc/bp_room.hip: one float64 accumulator per output sample, the taps added in ascending order, each step
the exact product of two float32 numbers added with one rounding.  That is the device's sequence of operations element for
element, so the tests compare with np.array_equal on the uint32 view."""
import numpy as np

import philox_np as PX

BLOCK = 2048          # outputs of one workgroup of bp_mix_reverb_fir (RV_BLOCK in csrc/bp_room.hip)
TAP_TILE = 256        # taps of one LDS tile (RV_TILE)
MAX_TAPS = 65536      # BP_MIX_RIR_MAX_TAPS
REVERBERANT, EARLY = 0, 1


def delay(h):
    """First index at which |h[j]| is largest."""
    return int(np.argmax(np.abs(np.asarray(h, np.float32))))


def shifted(s, k):
    """t[i] = s[i + k], zero outside the sentence."""
    n = s.size
    t = np.zeros(n, s.dtype)
    lo, hi = max(0, -k), min(n, n - k)
    if hi > lo:
        t[lo:hi] = s[lo + k:hi + k]
    return t


def reverb(s, h, early_taps):
    """(r, e) as float32; early_taps: one number, or a sequence (then e is a list, one per entry)."""
    s64 = np.asarray(s, np.float32).astype(np.float64)
    h = np.asarray(h, np.float32)
    many = np.ndim(early_taps) > 0
    taps = [int(t) for t in (early_taps if many else [early_taps])]
    d, Lh = delay(h), h.size
    acc = np.zeros(s64.size, np.float64)
    snap = [None] * len(taps)
    for j in range(Lh):
        acc += np.float64(h[j]) * shifted(s64, d - j)              # the whole sentence at once
        for k, t in enumerate(taps):
            if j == min(Lh - 1, d + t):
                snap[k] = acc.astype(np.float32)
    r = acc.astype(np.float32)
    return (r, snap) if many else (r, snap[0])


def pairs(seed, n_clean, n_rir):
    """pair_rir[c] = (philox(c, 0, 3, 0)[0] * n_rir) >> 32."""
    out = []
    for c in range(n_clean):
        w = PX.philox4x32_10(np.array([c], np.uint64), np.array([0], np.uint64), np.array([3], np.uint64), np.array([0], np.uint64),
                             seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        out.append((int(w[0][0]) * int(n_rir)) >> 32)
    return np.array(out, np.int32)


def exact_case(rng, n, Lh):
    """A sentence of half-integers and integer taps in [-2, 2] (the recipe of tests/exact_data.py): every partial sum is exact in
    float32, so any order of summation gives the same bits."""
    return (rng.integers(-64, 65, n) / 2.0).astype(np.float32), rng.integers(-2, 3, Lh).astype(np.float32)
