"""Simulated room impulse responses (include/bp_c_api.h) restated in float64 from the definition, calling
nothing in the library: the box loop over the images, the host tables B_d by repeated multiplication, the windowed sinc, fl32 at
the end; the seeded room draw on tests/philox_np.py; Eyring's formula; the fixture rooms of the tests.  Scalars that the C side
computes with libm (exp, log, sqrt, ceil) use `math` here, so that == holds for the host-only entry points."""
import math

import numpy as np

import philox_np as PH

C = 343.0
MAX_TAPS = 65536
MAX_IMAGES = 1 << 26
ROOM_DTYPE = np.dtype([("L", np.float64, 3), ("src", np.float64, 3), ("mic", np.float64, 3), ("beta", np.float64, 6)])
RANGES = dict(L_lo=(3.0, 3.0, 2.5), L_hi=(10.0, 8.0, 4.0), t60=(0.2, 0.8), margin=0.5, dist=(0.5, 3.0))


def room(L, src, mic, beta):
    r = np.zeros((), ROOM_DTYPE)
    r["L"], r["src"], r["mic"], r["beta"] = L, src, mic, beta
    return r


def d0(r):
    dx, dy, dz = (float(r["src"][d]) - float(r["mic"][d]) for d in range(3))
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def window_default(fs):
    return 2 * int(math.floor(0.004 * fs + 0.5))


def orders(r, fs, n_taps, Tw):
    reach = ((n_taps + Tw / 2.0) * C) / fs
    N = [int(math.ceil(reach / (2.0 * float(r["L"][d])))) for d in range(3)]
    return tuple(N), 8 * (2 * N[0] + 1) * (2 * N[1] + 1) * (2 * N[2] + 1)


def table(lo, hi, N):
    """B[n + N][p] = lo^|n-p| hi^|n|, each power by repeated multiplication from 1.0 (0^0 = 1)"""
    pl, ph = [1.0], [1.0]
    for _ in range(N + 1):
        pl.append(pl[-1] * lo)
        ph.append(ph[-1] * hi)
    return np.array([[pl[abs(n - p)] * ph[abs(n)] for p in (0, 1)] for n in range(-N, N + 1)], np.float64)


def window(u, Tw):
    """w(u) = 0.5 (1 + cos(2 pi u / Tw)) sinc(u) inside |u| < Tw/2, else 0; sinc(0) = 1"""
    u = np.asarray(u, np.float64)
    pu = np.pi * u
    safe = np.where(u == 0.0, 1.0, pu)
    sinc = np.where(u == 0.0, 1.0, np.sin(pu) / safe)
    return np.where(np.abs(u) < Tw / 2.0, 0.5 * (1.0 + np.cos(2.0 * np.pi * u / Tw)) * sinc, 0.0)


def images(r, fs, n_taps, Tw):
    """(tau, a) of every image of the box, in the library's documented order (axis 2 outermost, p after n on each axis)"""
    (N0, N1, N2), _ = orders(r, fs, n_taps, Tw)
    ax = []
    for d, N in enumerate((N0, N1, N2)):
        n = np.repeat(np.arange(-N, N + 1), 2).astype(np.float64)
        p = np.tile([0.0, 1.0], 2 * N + 1)
        x = (1.0 - 2.0 * p) * float(r["src"][d]) + 2.0 * n * float(r["L"][d]) - float(r["mic"][d])
        ax.append((x, table(float(r["beta"][2 * d]), float(r["beta"][2 * d + 1]), N).reshape(-1)))
    (x0, b0), (x1, b1), (x2, b2) = ax
    X2, X1, X0 = np.meshgrid(x2, x1, x0, indexing="ij")
    B2, B1, B0 = np.meshgrid(b2, b1, b0, indexing="ij")
    dist = np.sqrt((X0 * X0 + X1 * X1) + X2 * X2).reshape(-1)
    a = (((B0 * B1) * B2).reshape(-1)) * (d0(r) / dist)
    return dist * fs / C, a


def reaching(r, fs, n_taps, Tw):
    """the images whose window reaches a tap of [0, n_taps): (tau, a)"""
    tau, a = images(r, fs, n_taps, Tw)
    j_lo = np.maximum(np.ceil(tau - Tw / 2.0), 0)
    j_hi = np.minimum(np.floor(tau + Tw / 2.0), n_taps - 1)
    hit = np.zeros(tau.size, bool)
    for i in np.nonzero(j_hi >= j_lo)[0]:
        j = np.arange(int(j_lo[i]), int(j_hi[i]) + 1)
        hit[i] = bool(np.any(np.abs(j - tau[i]) < Tw / 2.0))
    return tau[hit], a[hit]


def response64(r, fs, n_taps, Tw):
    """sum over the images of a w(j - tau), float64 [n_taps], before fl32"""
    tau, a = images(r, fs, n_taps, Tw)
    h = np.zeros(n_taps, np.float64)
    j_lo = np.maximum(np.ceil(tau - Tw / 2.0), 0).astype(np.int64)
    j_hi = np.minimum(np.floor(tau + Tw / 2.0), n_taps - 1).astype(np.int64)
    for i in np.nonzero(j_hi >= j_lo)[0]:
        j = np.arange(j_lo[i], j_hi[i] + 1)
        h[j] += a[i] * window(j - tau[i], Tw)
    return h


def response(r, fs, n_taps, Tw):
    return response64(r, fs, n_taps, Tw).astype(np.float32)


def bar(ref64):
    """the tests' per-tap bar: one fp32 ulp of the reference (a rounding flip of fl32) + 1e-9 of the largest tap (the error of the
    double sums; the restatement itself is within 1e-13 of a long-double evaluation)"""
    ref32 = np.asarray(ref64, np.float64).astype(np.float32)
    return np.spacing(np.abs(ref32)).astype(np.float64) + 1e-9 * float(np.abs(ref64).max() if ref64.size else 0.0)


# ---- Eyring and the seeded draw
def beta_eyring(L, t60):
    L = [float(x) for x in L]
    V = (L[0] * L[1]) * L[2]
    S = 2.0 * ((L[0] * L[1] + L[0] * L[2]) + L[1] * L[2])
    k = (24.0 * math.log(10.0)) / C
    alpha = 1.0 - math.exp(-((k * V) / (S * float(t60))))
    return np.full(6, math.sqrt(1.0 - alpha), np.float64)


def _U(seed, r, a):
    w = PH.philox4x32_10([r], [a], [4], [0], seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [float(int(x[0])) / 4294967296.0 for x in w]


def rooms(seed, n, **ranges):
    """the rooms of bp_rir_rooms; raises ValueError naming the room when no attempt qualifies"""
    g = dict(RANGES, **ranges)
    out = np.zeros(n, ROOM_DTYPE)
    m = float(g["margin"])
    for r in range(n):
        u = _U(seed, r, 0)
        L = [float(g["L_lo"][d]) + u[d] * (float(g["L_hi"][d]) - float(g["L_lo"][d])) for d in range(3)]
        t60 = float(g["t60"][0]) + u[3] * (float(g["t60"][1]) - float(g["t60"][0]))
        u = _U(seed, r, 1)
        mic = [m + u[d] * (L[d] - 2.0 * m) for d in range(3)]
        for k in range(32):
            u = _U(seed, r, 2 + k)
            src = [m + u[d] * (L[d] - 2.0 * m) for d in range(3)]
            dx, dy, dz = (src[d] - mic[d] for d in range(3))
            dist = math.sqrt((dx * dx + dy * dy) + dz * dz)
            if float(g["dist"][0]) <= dist <= float(g["dist"][1]):
                break
        else:
            raise ValueError("room %d" % r)
        out[r] = room(L, src, mic, beta_eyring(L, t60))
    return out


def attempts(seed, r, **ranges):
    """the attempt (0 .. 31) room r's source comes from, or None"""
    g = dict(RANGES, **ranges)
    m = float(g["margin"])
    u = _U(seed, r, 0)
    L = [float(g["L_lo"][d]) + u[d] * (float(g["L_hi"][d]) - float(g["L_lo"][d])) for d in range(3)]
    u = _U(seed, r, 1)
    mic = [m + u[d] * (L[d] - 2.0 * m) for d in range(3)]
    for k in range(32):
        u = _U(seed, r, 2 + k)
        src = [m + u[d] * (L[d] - 2.0 * m) for d in range(3)]
        dx, dy, dz = (src[d] - mic[d] for d in range(3))
        if float(g["dist"][0]) <= math.sqrt((dx * dx + dy * dy) + dz * dz) <= float(g["dist"][1]):
            return k
    return None


def passes_image_checks(r, fs, n_taps, Tw):
    """the argument checks of bp_rir_image on one room"""
    vals = np.concatenate([r["L"], r["src"], r["mic"], r["beta"]])
    if not np.all(np.isfinite(vals)) or not (1000 <= fs <= 192000 and 2 <= Tw <= 1024 and 1 <= n_taps <= MAX_TAPS):
        return False
    ok = all(0.5 <= r["L"][d] <= 100.0 and 0.0 < r["src"][d] < r["L"][d] and 0.0 < r["mic"][d] < r["L"][d] for d in range(3))
    ok = ok and all(0.0 <= b <= 1.0 for b in r["beta"]) and d0(r) >= 0.05
    return bool(ok and orders(r, fs, n_taps, Tw)[1] <= MAX_IMAGES)


# ---- the fixtures of tests/test_rir_gpu.py: name -> (room, fs, taps, Tw)
_A = dict(L=(3.0, 2.5, 2.2), src=(1.1, 0.9, 1.3), mic=(2.2, 1.7, 0.9), beta=(0.9, 0.7, 0.8, 0.6, 0.5, 0.85))
_B = dict(L=(8.0, 2.0, 2.4), src=(1.0, 1.0, 1.2), mic=(7.0, 0.9, 1.3), beta=(0.9, 0.85, 0.9, 0.9, 0.8, 0.85))
_NEAR = dict(_A, mic=(1.1 + 0.05, 0.9, 1.3))                    # the microphone 0.05 m from the source


def fixtures():
    return {
        "a": (room(**_A), 8000, 300, 64),                       # N = (3, 3, 4): several chunks, a ragged last one
        "b": (room(**_B), 16000, 517, 33),                      # orders differ per axis, odd window, taps no multiple of the block
        "c": (room(**dict(_A, beta=(0.0, 1.0, 0.8, 0.6, 0.5, 0.85))), 8000, 64, 64),   # a wall that kills images, one that keeps them
        "d": (room(**_NEAR), 8000, 257, 64),                    # the window straddles tap 0
        "e": (room(**_NEAR), 8000, 1, 64),
        "f": (room(**_B), 8000, 120, 16),                       # nothing arrives: all zeros
        "g": (room(**_A), 16000, 1200, 64),                     # thousands of images, several tap blocks
    }


FIXTURE_ORDER = "abcdefg"
