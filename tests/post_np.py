"""NumPy restatement of the post-processing of the LPS estimate (include/bp_c_api.h): the post-processed value,
the 64-part sums of bp_gv_mix and the factors of bp_gv_factors.  Written from the definition, not from the sources.

Every step of the value is one multiply, add or subtract of float32 values, and numpy rounds each float32 operation once: the bits
are those of the device.  The sums are a Python loop of float64 additions in the defined order."""
import numpy as np

F32 = np.float32
PARTS = 64


def gate(m, lo, hi):
    """u in [0, 1] from the mask estimate: the ramp between lo and hi (a NaN mask gives 0), or the step at hi when hi == lo."""
    m = np.asarray(m, F32)
    lo, hi = F32(lo), F32(hi)
    if hi > lo:
        inv = F32(1.0 / (float(hi) - float(lo)))
        u = (m - lo) * inv
        with np.errstate(invalid="ignore"):
            return np.where(u > 0, np.where(u < 1, u, F32(1)), F32(0)).astype(F32)
    with np.errstate(invalid="ignore"):
        return np.where(m >= hi, F32(1), F32(0)).astype(F32)


def post(x, y=None, m=None, center=None, scale=None, lo=0.5, hi=0.5, weight=1.0):
    """The post-processed rows: GV with center / scale when given, then the gate when a mask block m is given.
    x, y, m: [n][D] float32."""
    x = np.asarray(x, F32)
    if center is not None:
        c, s = np.asarray(center, F32), np.asarray(scale, F32)
        d = x - c
        t = s * d
        x = c + t
    if m is not None:
        u = gate(m, lo, hi)
        w = F32(weight) * u
        e = np.asarray(y, F32) - x
        q = w * e
        x = x + q
    return x.astype(F32)


def part_sums(v):
    """(sum, sum of squares) of the rows v [n][D] in bp_gv_mix's order, float64 [D] each."""
    v = np.asarray(v, F32).astype(np.float64)
    n, D = v.shape
    q = (n + PARTS - 1) // PARTS
    tot1, tot2 = None, None
    for p in range(PARTS):
        a1, a2 = np.zeros(D), np.zeros(D)
        for g in range(p * q, min(n, (p + 1) * q)):
            a1 = a1 + v[g]
            a2 = a2 + v[g] * v[g]
        tot1 = a1 if p == 0 else tot1 + a1
        tot2 = a2 if p == 0 else tot2 + a2
    return tot1, tot2


def gv_sums(est, ref):
    """The dictionary of BP_GPU.gv_mix from the estimate rows and the clean LPS rows of one call."""
    e1, e2 = part_sums(est)
    r1, r2 = part_sums(ref)
    return {"est_sum": e1, "est_sq": e2, "ref_sum": r1, "ref_sq": r2, "frames": int(np.asarray(est).shape[0])}


def gv_factors(stats, mode="indep"):
    """(center, scale), float32 [D]: scaling about the clean mean; "dep": sqrt(vr / ve) per bin; "indep": sqrt(D / sum ve / vr)."""
    n = float(stats["frames"])
    if stats["frames"] < 2:
        raise ValueError("frames < 2")
    e1, e2, r1, r2 = (np.asarray(stats[k], np.float64) for k in ("est_sum", "est_sq", "ref_sum", "ref_sq"))
    me, mr = e1 / n, r1 / n
    ve, vr = e2 / n - me * me, r2 / n - mr * mr
    if not (np.all(ve > 0) and np.all(vr > 0)):
        raise ValueError("variance <= 0")
    D = e1.size
    if mode == "dep":
        scale = np.sqrt(vr / ve).astype(F32)
    else:
        pooled = 0.0
        for k in range(D):
            pooled = pooled + ve[k] / vr[k]
        scale = np.full(D, F32(np.sqrt(D / pooled)), F32)
    return mr.astype(F32), scale
