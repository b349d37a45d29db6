"""Each bf16 step kernel alone, on operands that are known by construction, held to float64 at half-ulp bars (plain Python; nothing
from the product is imported).  tests/test_bf16_iso_host.py proves the constructions on the CPU with the numpy model below,
tests/test_bf16_iso_gpu.py (-m gpu) holds the device to the bars; DESIGN.md 2 has the paragraph that goes with it.

Why.  tests/test_dispatch_gpu.py compares whole bf16 nets with another bf16 implementation (2e-3 forward, 2e-2 rms gradients: two
correct implementations differ by that much); tests/test_exact_gpu.py is bit for bit, but on few-bit data where no bf16 store ever
rounds; bp_read_layer_output refuses bf16 handles.  A store that truncates, rounds before the bias, takes act' from the wrong copy
or writes a transposed copy one value off on generic data passes all of them.

How.  Kernel selection depends on (Bp, ld[l-1], ld[l], position, logistic) only (tests/dispatch_np.py), never on the data.  Every
case is a small net that dispatches the kernel under test at one layer, and whose other layers are arithmetically transparent:

  gather layer      W[p][c] = 1 where p == c (an identity; bias 0, ReLU, inputs >= 0): y_l = y_{l-1} exactly in any summation order
                    (one non-zero product plus zeros).  As the linear output layer it returns a hidden bf16 tensor through forward().
  one-hot rows      y_{l-1}[f][p] = delta(p, pi(f)), pi injective: G_l[pi(f)][c] = dx_l[f][c] exactly.  grads_resident + read_grads
                    returns a hidden bf16 delta elementwise -- through the TRANSPOSED copies, which the weight gradient reads.
  snapped deltas    t = o_dev - d Bg/2, o_dev the handle's own forward() of the bunch, d a bf16 number of six significant bits,
                    2^-4 <= |d| < 2: bf16(fl32(2/Bg) fl32(o - t)) = d whatever the last bits of o (tests/exact_data.py).

Generic operands are normal draws rounded to bf16 (full significands), inputs of unit scale, weights 1/sqrt(K), magnitudes floored
so that no operand or product is below 2^-20.  Every layer that carries a one-hot or a gathered tensor is at least as wide as the
bunch, so no frame has to wait for a second pass.

Families: C bp_to_bf16_both, both copies | F hidden forward, yb through forward() | T its transposed copy ybT through
G_2 | O output forward (fp32) | E output delta store, dxbT through G_L and the bias sum | D dgrad, dxbT_1 through G_1 | W weight-
gradient store + bias sums | U the fused update.

Bars -- nothing is tuned on the device.
  rho-bar (fp32 results): |got - ref64| <= 4 rho_ref (sum_k |a_k b_k| + |bias|); rho_ref = max |z32 - z64| / sum|ab| over a 64 x 64
      sample block of that GEMM, z32 the k-ordered fp32 chain of the same operands (rho_ref); 4 x for another summation order.
  half-ulp bar (bf16 results, against the REAL value): |got - v64| <= ulp_bf16(v64)/2 + slack, slack = the rho-bar of the
      accumulation inside times the Lipschitz factor of what follows (1 ReLU and dgrad, 1/4 Sigmoid, scale for the output delta);
      got must be a bf16 number.
  sigmoid term: 4 x the largest |fp32 1/(1+exp(-z)) - float64| of numpy on the case's own z, additive.
No element is excluded."""
import collections
import zlib

import numpy as np

import dispatch_np as D
from torch_ref import bf16_round

LR, MOM, WC = 0.5, 0.5, 0.0
MARGIN = 4.0
U24 = 2.0 ** -24

Iso = collections.namedtuple("Iso", ["id", "family", "ls", "B", "act", "out", "layer", "kernel", "why"])

# (bunch, width) that takes the hidden forward (N = width) and the dgrad (prev = width) to each tile form
ROWS = collections.OrderedDict([("r32", (40, 130)), ("r64", (1040, 2000)), ("r128", (1000, 2100)), ("r128dma", (1000, 2048))])
BM = {"r32": 32, "r64": 64, "r128": 128, "r128dma": 128}
# [K, K, N] at bunch B for each output-forward form; K >= B so that family E can run one-hot rows through layer 1
OUTS = collections.OrderedDict([("o32", (40, 100, 130, 32, 1)), ("o32ks4", (120, 1024, 100, 32, 4)), ("o64", (1040, 1100, 2000, 64, 1)),
                                ("o128", (1000, 1024, 2000, 128, 1))])
# [P, P, N] at bunch B for each weight-gradient form: LDS-DMA at padded bunch 128 .. 1024, generic 32 / 64 / 128-row tiles
WGRADS = collections.OrderedDict([("dma128", (120, 100, 130)), ("dma256", (200, 130, 70)), ("dma512", (500, 130, 70)), ("dma1024", (1000, 130, 70)),
                                  ("g32", (40, 100, 130)), ("g64", (48, 2100, 1000)), ("g128", (48, 2048, 1000))])


def _cases():
    out = []
    out.append(Iso("C_convert", "C", [130, 130, 130], 40, 0, None, 0, "bp_to_bf16_both", "fp32 -> bf16 of the input bunch: ties, neighbours of ties, largest finite"))
    for r, (B, n) in ROWS.items():
        k = 520 if r == "r128dma" else (100 if r == "r32" else 130)         # DMA form: 9 k-tiles, the ring of 4 wraps
        for act in (0, 1):
            out.append(Iso("F_%s_%s" % (r, "sigmoid" if act else "relu"), "F", [k, n, n], B, act, None, 1,
                           D.n_bf(D.BEPI_FWD_HIDDEN, BM[r], True, r == "r128dma"), "yb[1] through an identity output layer"))
            out.append(Iso("T_%s_%s" % (r, "sigmoid" if act else "relu"), "T", [k, n, n], B, act, None, 1,
                           D.n_bf(D.BEPI_FWD_HIDDEN, BM[r], True, r == "r128dma"), "ybT[1] through G_2 against one-hot output deltas"))
    for o, (B, k, n, bm, ks) in OUTS.items():
        for logi in (False, True):
            epi = D.BEPI_FWD_OUT_LOGI if logi else D.BEPI_FWD_OUT
            tag = "_logistic" if logi else ""
            out.append(Iso("O_%s%s" % (o, tag), "O", [k, k, n], B, 0, (n // 2 + 1, 0) if logi else None, 2, D.n_bf(epi, bm, True, False, ks),
                           "fp32 output of the output forward"))
            for loss in ((0, 1) if logi else (0,)):
                out.append(Iso("E_%s%s%s" % (o, tag, "_mse" if loss else ""), "E", [k, k, n], B, 0, (n // 2 + 1, loss) if logi else None, 2,
                               D.n_bf(epi, bm, True, False, ks), "dxbT[L] through G_L against one-hot rows, dxb[L] or dxbT[L] through the bias sum"))
    for r, (B, p) in ROWS.items():
        s0, n = {"r32": (50, 100), "r64": (1100, 130), "r128": (1000, 130), "r128dma": (1000, 520)}[r]      # DMA form: k = 576, 9 k-tiles
        out.append(Iso("D_%s_relu" % r, "D", [s0, p, n], B, 0, None, 2, D.n_bf(D.BEPI_DGRAD, BM[r], False, r == "r128dma"),
                       "dxbT[1] through G_1 against a one-hot input"))
    out.append(Iso("D_r32_sigmoid", "D", [50, 130, 100], 40, 1, None, 2, D.n_bf(D.BEPI_DGRAD, 32, False), "the same with y (1 - y) from the observed yb[1]"))
    for w, (B, p, n) in WGRADS.items():
        dma = w.startswith("dma")
        bm = {"g32": 32, "g64": 64, "g128": 128}.get(w)
        out.append(Iso("W_%s" % w, "W", [p, p, n], B, 0, None, 2, D.n_bf_store(D.pad64(B)) if dma else D.n_bf(D.BEPI_WGRAD_STORE, bm, False),
                       "G_2 and gb_2 from known y_1 and snapped dx_2"))
        out.append(Iso("U_%s" % w, "U", [p, p, n], B, 0, None, 2, D.n_bf_six(D.pad64(B)) if dma else D.n_bf(D.BEPI_WGRAD_UPDATE, bm, False),
                       "one fused step from zero momentum against the float64 update of the float64 G_2"))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
# the epilogue numbers a family may claim (check 4 of the host test)
FAMILY_EPI = {"F": (D.BEPI_FWD_HIDDEN,), "T": (D.BEPI_FWD_HIDDEN,), "O": (D.BEPI_FWD_OUT, D.BEPI_FWD_OUT_LOGI), "E": (D.BEPI_FWD_OUT, D.BEPI_FWD_OUT_LOGI),
              "D": (D.BEPI_DGRAD,), "W": (D.BEPI_WGRAD_STORE,), "U": (D.BEPI_WGRAD_UPDATE,)}
HALF_ULP_FAMILIES = ("F", "E", "D")


def launch_at(c):
    """The name dispatch_np puts at the layer and call the case says it tests."""
    cfg = D.Config(c.ls, c.B, 1, 1 if c.out else 0)
    if c.family in ("F", "T", "O", "E"):
        return D.fwd_bf16(cfg, c.layer).name
    if c.family == "D":
        return D.dgrad_bf16(cfg, c.layer).name
    if c.family in ("W", "U"):
        ws = D.wgrads_bf16(cfg, c.family == "U")
        return ws[0].name if cfg.bf_dma_ok() else ws[c.layer - 1].name
    return c.kernel


# ------------------------------------------------------------------ numbers
def f32(a):
    return np.asarray(a, np.float32)


def f64(a):
    return np.asarray(a, np.float64)


def is_bf16(a):
    return not (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF)).any()


def ulp_bf16(v):
    """The spacing of bf16 numbers at |v| (float64 in, 0 at 0): 2^(e - 8) for v = m 2^e, 1/2 <= m < 1."""
    m, e = np.frexp(np.abs(f64(v)))
    return np.where(m == 0, 0.0, np.ldexp(1.0, e - 8))


def ulp_f32(v):
    return np.spacing(np.abs(f32(v))).astype(np.float64)


def sigmoid32(z):
    with np.errstate(over="ignore"):
        return np.float32(1.0) / (np.float32(1.0) + np.exp(-f32(z)))


def sigmoid64(z):
    return 1.0 / (1.0 + np.exp(-f64(z)))


def sigmoid_term(z64):
    """4 x the largest error of numpy's fp32 1/(1 + exp(-z)) against float64 on these z."""
    z = f32(z64)
    return MARGIN * float(np.abs(sigmoid32(z).astype(np.float64) - sigmoid64(z)).max())


def rho_ref(A, Bm, add=None):
    """max |z32 - z64| / (sum_k |a b| + |add|) over the first 64 x 64 block of A . B (+ add), z32 the k-ordered fp32 chain.  (A
    product of fewer than 64 rows -- a bias sum has one -- takes more columns instead: 4096 elements.)"""
    A = f64(A)[:64]
    nc = 4096 // A.shape[0]
    Bm = f64(Bm)[:, :nc]
    a32, b32 = f32(A), f32(Bm)
    z = np.zeros((A.shape[0], Bm.shape[1]), np.float32)
    for k in range(A.shape[1]):
        z += a32[:, k:k + 1] * b32[k:k + 1]
    mag = np.abs(A) @ np.abs(Bm)
    z64 = A @ Bm
    if add is not None:
        z = z + f32(add)[:64, :nc]
        z64 = z64 + f64(add)[:64, :nc]
        mag = mag + np.abs(f64(add)[:64, :nc])
    return float((np.abs(z.astype(np.float64) - z64) / np.maximum(mag, 1e-300)).max())


def generic(rng, shape, scale=1.0, positive=False):
    """Normal draws of the scale, rounded to bf16, magnitudes floored at scale 2^-6."""
    v = rng.normal(size=shape) * scale
    s = np.where(v < 0, -1.0, 1.0)
    v = bf16_round(np.maximum(np.abs(v), scale * 2.0 ** -6).astype(np.float32))
    return (v if positive else s * v).astype(np.float32)


def snapped(rng, shape):
    """bf16 numbers of six significant bits, 2^-4 <= |d| < 2, random signs, exponents and mantissas."""
    d = rng.integers(32, 64, size=shape) / 32.0 * 2.0 ** rng.integers(-4, 1, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    return d.astype(np.float32)


def snap_targets(o_dev, d, Bg):
    """t = o_dev - d Bg/2 as fp32."""
    return (f64(o_dev) - f64(d) * (Bg / 2.0)).astype(np.float32)


def tie_distance(o_dev, t, d, Bg):
    """(distance of fl32(2/Bg) fl32(o - t) to the nearest bf16 tie) / (its fp32 perturbation: what 2 ulps of the product and one
    of o can move it by), smallest over the elements.  The host test asks 2^8."""
    s = np.float32(2.0) / np.float32(Bg)
    v = (s * (f32(o_dev) - f32(t))).astype(np.float64)
    u = ulp_bf16(v)
    tie = np.abs(np.abs(v - f64(d)) - u / 2)                          # d is a bf16 number: the ties beside it are d +- u/2
    pert = 2 * ulp_f32(v) + float(s) * ulp_f32(o_dev)
    return float((tie / pert).min())


def eye(k):
    return np.eye(k, dtype=np.float32)


# ------------------------------------------------------------------ data
class _Bag(object):
    pass


_PROBLEMS = {}


def _rng(c, salt=0):
    return np.random.default_rng(zlib.crc32(("%s %s %d" % (c.ls, c.B, c.act)).encode()) + salt)


def tie_inputs(rng, shape):
    """fp32 values >= 0 for family C: generic fp32, then by turns an exact tie with an even and with an odd lower neighbour, the
    fp32 numbers just below and just above such ties, the largest fp32 number that still rounds to a finite bf16, the largest
    bf16 number, and zero.  Returns (x, kind): kind 1 / 2 marks ties (even / odd lower neighbour)."""
    x = np.abs(rng.normal(size=shape)).astype(np.float32) + np.float32(2.0 ** -6)
    u = x.view(np.uint32).reshape(-1).copy()
    kind = np.zeros(u.size, np.int8)
    i = np.arange(u.size)
    hi = u & np.uint32(0xFFFE0000)                                     # even bf16 significand
    for r, (word, k) in enumerate([(hi | np.uint32(0x8000), 1), (hi | np.uint32(0x18000), 2), (hi | np.uint32(0x7FFF), 0), (hi | np.uint32(0x8001), 0),
                                   (hi | np.uint32(0x17FFF), 0), (hi | np.uint32(0x18001), 0)]):
        m = i % 16 == r
        u[m], kind[m] = word[m], k
    u[i % 257 == 100], kind[i % 257 == 100] = np.uint32(0x7F7F7FFF), 0
    u[i % 257 == 101], kind[i % 257 == 101] = np.uint32(0x7F7F0000), 0
    u[i % 257 == 102], kind[i % 257 == 102] = np.uint32(0), 0
    return u.view(np.float32).reshape(shape), kind.reshape(shape)


def problem(cid):
    """The data of a case, made once and read-only: W, b (fp32, index 0 unused) and x; per family pi (one-hot row -> unit), kappa
    (frame -> output column), d (snapped deltas), t (generic targets), kind (family C)."""
    if cid in _PROBLEMS:
        return _PROBLEMS[cid]
    c = BY_ID[cid]
    p, rng = _Bag(), _rng(c)
    s0, s1, s2 = c.ls
    B = c.B
    z = lambda n: np.zeros(n, np.float32)
    w = lambda k, n: generic(rng, (k, n), 1.0 / np.sqrt(k))
    if c.family == "C":
        p.W, p.b = [None, eye(s0), eye(s0)], [None, z(s1), z(s2)]
        p.x, p.kind = tie_inputs(rng, (B, s0))
        free, p.kappa = list(rng.permutation(s0)), []                   # a column of its own per frame, with a moderate positive input
        for f in range(B):
            k = next(k for k in free if 2.0 ** -6 <= p.x[f, k] < 8.0)
            free.remove(k)
            p.kappa.append(k)
        p.kappa = np.array(p.kappa)
    elif c.family in ("F", "T"):
        p.W, p.b = [None, w(s0, s1), eye(s1)], [None, generic(rng, s1, 0.5), z(s2)]
        p.x = generic(rng, (B, s0))
        p.kappa = rng.permutation(s2)[:B]
    elif c.family in ("O", "E", "W", "U"):
        p.W, p.b = [None, eye(s0), w(s1, s2)], [None, z(s1), generic(rng, s2, 0.5)]
        if c.family == "E":
            p.pi = rng.permutation(s0)[:B]
            p.x = np.zeros((B, s0), np.float32)
            p.x[np.arange(B), p.pi] = 1.0
            p.t = rng.normal(size=(B, s2)).astype(np.float32)
            if c.out:
                p.t[:, c.out[0]:] = rng.random((B, s2 - c.out[0])).astype(np.float32)
        else:
            p.x = generic(rng, (B, s0), positive=True)
            p.d = snapped(rng, (B, s2))
    elif c.family == "D":
        p.W, p.b = [None, w(s0, s1), w(s1, s2)], [None, z(s1), generic(rng, s2, 0.5)]
        p.pi = rng.permutation(s0)[:B]
        p.x = np.zeros((B, s0), np.float32)
        p.x[np.arange(B), p.pi] = 1.0
        p.d = snapped(rng, (B, s2))
    for v in p.__dict__.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _PROBLEMS[cid] = p
    return p


# ------------------------------------------------------------------ checks
Check = collections.namedtuple("Check", ["name", "got", "ref", "bar", "bf16", "live"])


def check(name, got, ref, bar=None, bf16=False, live=None):
    """bar None: bit for bit.  Else an array (or scalar) of per-element bounds on |got - ref|.  bf16: got must be bf16 numbers."""
    return Check(name, np.asarray(got), np.asarray(ref), bar, bf16, live)


def ratio_of(ch):
    """(largest |got - ref| / bar over the elements -- 0 where both are 0, inf where only the bar is; bit for bit: 0 or inf --, the
    per-element ratios)."""
    g, r = np.atleast_1d(f64(ch.got)), np.atleast_1d(f64(ch.ref))
    if g.shape != r.shape:
        return float("inf"), None
    err = np.abs(g - r)
    err[~np.isfinite(err)] = np.inf
    if ch.bar is None:
        ne = np.atleast_1d(f32(ch.got)) != np.atleast_1d(f32(ch.ref))
        return (float("inf") if ne.any() else 0.0), np.where(ne, np.inf, 0.0)
    bar = np.broadcast_to(f64(ch.bar), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bar)
    q = np.where(np.isnan(q), np.inf, q)
    worst = float(q.max()) if q.size else 0.0
    if ch.bf16 and not is_bf16(ch.got):
        worst = float("inf")
    return worst, q


def share_over(ch):
    """The share of the live elements of a check that miss its bar."""
    _, q = ratio_of(ch)
    live = np.ones(q.shape, bool) if ch.live is None else ch.live
    return float((q[live] > 1.0).mean())


class Result(object):
    def __init__(self):
        self.checks, self.claims, self.figures = [], [], {}

    def ratios(self):
        return {ch.name: ratio_of(ch)[0] for ch in self.checks}


def pads_are_zero(res, c, pw, pb, layers):
    for l in layers:
        prev, cur = c.ls[l - 1], c.ls[l]
        pads = int(np.count_nonzero(pw[l][prev:, :])) + int(np.count_nonzero(pw[l][:, cur:])) + int(np.count_nonzero(pb[l][cur:]))
        res.checks.append(check("pad words of layer %d that are not 0.0" % l, np.float32(pads), np.float32(0)))


def half_ulp(v64, slack):
    return ulp_bf16(v64) / 2 + slack


# ------------------------------------------------------------------ the families
def run_C(c, p, dev, make):
    res = Result()
    o = dev.forward(p.x)
    res.checks.append(check("forward = bf16_rne(x)", o, bf16_round(p.x)))
    # the transposed copy: dx_2 = 1 at [f][kappa(f)] passes the identity dgrad where y_1[f][kappa(f)] > 0, so G_1[p][kappa(f)] = yb0[f][p]
    B, n = c.B, c.ls[0]
    t, fr = o.copy(), np.arange(c.B)
    t[fr, p.kappa] = (f64(o[fr, p.kappa]) - B / 2.0).astype(np.float32)
    pw, pb = dev.grads(p.x, t)
    G = pw[1][:n, :n]
    obs = G[:, p.kappa].T
    other = np.ones(n, bool)
    other[p.kappa] = False
    res.checks += [check("ybT0 through G1 = yb0 through forward", obs, o), check("columns of G1 without a frame", G[:, other], 0 * G[:, other])]
    pads_are_zero(res, c, pw, pb, (1, 2))
    res.claims += [("yb0", o), ("ybT0", obs)]
    return res


def _hidden_ref(c, p):
    """float64 value and half-ulp bar of yb[1] = act(x . W1 + b1) of an F / T / D net."""
    x, W1, b1 = f64(p.x), f64(p.W[1]), f64(p.b[1])
    z = x @ W1 + b1
    rho = rho_ref(p.x, p.W[1], np.broadcast_to(p.b[1], (p.x.shape[0], b1.size)))
    zbar = MARGIN * rho * (np.abs(x) @ np.abs(W1) + np.abs(b1))
    if c.act == 0:
        return np.maximum(z, 0.0), zbar, rho, 0.0, z
    st = sigmoid_term(z)
    return sigmoid64(z), 0.25 * zbar + st, rho, st, z


def run_F(c, p, dev, make):
    res = Result()
    o = dev.forward(p.x)
    v, slack, rho, st, z = _hidden_ref(c, p)
    res.checks.append(check("yb1", o, v, half_ulp(v, slack), bf16=True, live=z > 0 if c.act == 0 else None))
    res.claims.append(("yb1", o))
    res.figures.update(rho_ref=rho, sigmoid_term=st, slack_share=float((slack < ulp_bf16(v) / 8)[v != 0].mean()), relu_live=float((z > 0).mean()),
                       dead_blocks=len(dead_blocks(v)))
    return res


def run_T(c, p, dev, make):
    res = Result()
    B, n = c.B, c.ls[2]
    o = dev.forward(p.x)
    t = o.copy()
    fr = np.arange(B)
    t[fr, p.kappa] = (f64(o[fr, p.kappa]) - B / 2.0).astype(np.float32)              # dx_L = 1 at [f][kappa(f)], exactly 0 elsewhere
    pw, pb = dev.grads(p.x, t)
    G = pw[2][:n, :n]
    obs = G[:, p.kappa].T
    other = np.ones(n, bool)
    other[p.kappa] = False
    one = np.zeros(n, np.float32)
    one[p.kappa] = 1.0
    res.checks += [check("ybT1 through G2 = yb1 through forward", obs, o), check("columns of G2 without a frame", G[:, other], 0 * G[:, other]),
                   check("gb2", pb[2][:n], one)]
    pads_are_zero(res, c, pw, pb, (1, 2))
    res.claims += [("yb1", o), ("ybT1", obs)]
    return res


def _out_ref(c, p):
    x, W2, b2 = f64(p.x), f64(p.W[2]), f64(p.b[2])
    z = x @ W2 + b2
    rho = rho_ref(p.x, p.W[2], np.broadcast_to(p.b[2], (p.x.shape[0], b2.size)))
    return z, MARGIN * rho * (np.abs(x) @ np.abs(W2) + np.abs(b2)), rho


def run_O(c, p, dev, make):
    res = Result()
    o = dev.forward(p.x)
    z, bar, rho = _out_ref(c, p)
    lin = c.ls[2] if c.out is None else c.out[0]
    res.checks.append(check("output, linear columns", o[:, :lin], z[:, :lin], bar[:, :lin]))
    if c.out:
        st = sigmoid_term(z[:, lin:])
        res.checks.append(check("output, logistic columns", o[:, lin:], sigmoid64(z[:, lin:]), bar[:, lin:] + st))
        res.figures["sigmoid_term"] = st
    res.claims.append(("yb1", p.x))
    res.figures["rho_ref"] = rho
    return res


def _bias_sum_check(name, got, dx):
    """A bias gradient against the column sums of the observed deltas, at the rho-bar of that sum."""
    dx = f64(dx)
    rho = rho_ref(np.ones((1, dx.shape[0])), dx)
    mag = np.abs(dx).sum(0)
    return check(name, got, dx.sum(0), np.maximum(MARGIN * rho * mag, U24 * mag * ~order_free(dx))), rho


def order_free(dx):
    """Per column: whether sum |dx| is below 2^24 quanta of the column (the largest power of two that divides its terms), so that
    every partial sum in every order is an fp32 number (condition (a) of tests/exact_data.py).  Where it is, a measured rho_ref
    of 0 is a promise for any order; where it is not, some order rounds at least once, and the bar is no less than one rounding
    unit of the magnitude -- the k-ordered chain of a 40-frame sum can come out exact by luck."""
    dx = np.abs(f64(dx))
    m, e = np.frexp(np.where(dx == 0, 1.0, dx))
    i = np.ldexp(m, 53).astype(np.int64)
    low = np.log2((i & -i).astype(np.float64)).astype(np.int64)
    q = np.ldexp(1.0, np.where(dx == 0, 1024, e - 53 + low).min(0))
    return dx.sum(0) / q < 2.0 ** 24


def dead_blocks(v):
    """The 64 x 64 blocks of v without a non-zero element."""
    v = np.asarray(v)
    return [(i, j) for i in range(0, v.shape[0], 64) for j in range(0, v.shape[1], 64) if not v[i:i + 64, j:j + 64].any()]


def smallest_operands(c, p):
    """(smallest non-zero |a|, smallest non-zero |b|) of the GEMM under test: no operand and no product below 2^-20."""
    a, b = {"F": (p.x, p.W[1]), "T": (p.x, p.W[1]), "O": (p.x, p.W[2]), "E": (p.x, p.W[2]), "W": (p.x, getattr(p, "d", None)),
            "U": (p.x, getattr(p, "d", None)), "D": (getattr(p, "d", None), p.W[2]), "C": (p.x, p.W[1])}[c.family]
    nz = lambda v: float(np.abs(v)[np.asarray(v) != 0].min())
    return nz(a), nz(b)


def run_E(c, p, dev, make):
    res = Result()
    B, n = c.B, c.ls[2]
    o = dev.forward(p.x)
    pw, pb = dev.grads(p.x, p.t)
    G = pw[2][:c.ls[1], :n]
    obs = G[p.pi]
    s = float(np.float32(2.0) / np.float32(B))
    v = s * (f64(o) - f64(p.t))
    roundings = 4.0                                                     # two fp32 roundings (o - t, the product), twice
    if c.out and c.out[1] == 1:
        lin = c.out[0]
        v[:, lin:] *= f64(o[:, lin:]) * (1.0 - f64(o[:, lin:]))
        roundings = 10.0                                                # and 1 - o, o (1 - o), the product
    slack = roundings * U24 * np.abs(v)
    other = np.ones(c.ls[1], bool)
    other[p.pi] = False
    res.checks += [check("dxbT%d through G%d" % (2, 2), obs, v, half_ulp(v, slack), bf16=True), check("rows of G2 without a frame", G[other], 0 * G[other])]
    gb, rho = _bias_sum_check("gb2 = column sums of the observed dx2", pb[2][:n], obs)
    res.checks.append(gb)
    pads_are_zero(res, c, pw, pb, (1, 2))
    res.claims += [("ybT1", p.x), ("dxbT2", obs)]
    res.figures.update(rho_ref_bias_sum=rho, slack_share=float((slack < ulp_bf16(v) / 8).mean()))
    return res


def run_D(c, p, dev, make):
    res = Result()
    B, (s0, s1, s2) = c.B, c.ls
    o = dev.forward(p.x)
    if c.act == 0:
        y1 = np.maximum(p.W[1][p.pi], np.float32(0.0))                # relu(1 . W1b[pi(f)] + 0): one product, exact
    else:                                                             # Sigmoid: yb[1] observed as in family F, by the same kernel at the same shape
        twin = make([s0, s1, s1], B, c.act, None, [None, p.W[1], eye(s1)], [None, p.b[1], np.zeros(s1, np.float32)])
        try:
            y1 = twin.forward(p.x)
        finally:
            twin.close()
    t = snap_targets(o, p.d, B)
    pw, pb = dev.grads(p.x, t)
    G = pw[1][:s0, :s1]
    obs = G[p.pi]
    d, W2 = f64(p.d), f64(p.W[2])
    a = d @ W2.T
    rho = rho_ref(p.d, p.W[2].T)
    abar = MARGIN * rho * (np.abs(d) @ np.abs(W2.T))
    y = f64(y1)
    if c.act == 0:
        actp, extra = (y > 0).astype(np.float64), 0.0
    else:
        actp, extra = (1.0 - y) * y, 4.0 * U24                           # 1 - y, (1 - y) y and the product, in fp32
    v = actp * a
    slack = actp * abar + extra * np.abs(v)
    other = np.ones(s0, bool)
    other[p.pi] = False
    res.checks += [check("dxbT1 through G1", obs, v, half_ulp(v, slack), bf16=True, live=actp > 0), check("rows of G1 without a frame", G[other], 0 * G[other])]
    gb, rho_b = _bias_sum_check("gb1 = column sums of the observed dx1", pb[1][:s1], obs)
    res.checks.append(gb)
    pads_are_zero(res, c, pw, pb, (1, 2))
    res.claims += [("yb1", y1), ("dxb2", p.d), ("dxbT1", obs)]
    res.figures.update(rho_ref=rho, rho_ref_bias_sum=rho_b, relu_live=float((actp > 0).mean()), tie_distance=tie_distance(o, t, p.d, B),
                       slack_share=float((slack < ulp_bf16(v) / 8)[v != 0].mean()), dead_blocks=len(dead_blocks(v)))
    return res


def _wgrad_ref(c, p):
    x, d = f64(p.x), f64(p.d)
    rho = rho_ref(p.x.T, p.d)
    rho_b = rho_ref(np.ones((1, c.B)), p.d)
    return x.T @ d, MARGIN * rho * (np.abs(x).T @ np.abs(d)), d.sum(0), MARGIN * rho_b * np.abs(d).sum(0), rho, rho_b


def run_W(c, p, dev, make):
    res = Result()
    o = dev.forward(p.x)
    t = snap_targets(o, p.d, c.B)
    pw, pb = dev.grads(p.x, t)
    G, Gbar, gb, gbbar, rho, rho_b = _wgrad_ref(c, p)
    res.checks += [check("G2", pw[2][:c.ls[1], :c.ls[2]], G, Gbar), check("gb2", pb[2][:c.ls[2]], gb, gbbar)]
    pads_are_zero(res, c, pw, pb, (1, 2))
    res.claims += [("ybT1", p.x), ("dxbT2", p.d), ("dxb2", p.d)]
    res.figures.update(rho_ref=rho, rho_ref_bias_sum=rho_b, tie_distance=tie_distance(o, t, p.d, c.B))
    return res


def run_U(c, p, dev, make):
    """dW = m 0 - c1 (G / B + wc W), W' = W + dW with c1 = (1 - m) lr (tests/update_cases.py has the restatement)."""
    import update_cases as UC
    res = Result()
    o = dev.forward(p.x)
    t = snap_targets(o, p.d, c.B)
    W, b, dW, db = dev.train(p.x, t)
    G, Gbar, gb, gbbar, rho, rho_b = _wgrad_ref(c, p)
    h = UC.Hyper("iso", 0, MOM, WC, LR)
    z = lambda a: np.zeros_like(f64(a))
    Dn, dn, Wn, bn = UC.restate(h, c.B, [None, p.W[2]], [None, p.b[2]], [None, z(p.W[2])], [None, z(p.b[2])], [None, G], [None, gb])
    coef = (1.0 - MOM) * LR / c.B
    # the momentum state: the rho-bar scaled by the update's coefficient + 2 fp32 ulps of the result.  W' = W + dW carries dW's error
    # through one more rounded addition: dW's bar + 2 ulps of W' (where the two cancel, 2 ulps of W' alone is less than the half ulp
    # of dW that correctly rounded fp32 arithmetic leaves)
    dWbar, dbbar = coef * Gbar + 2 * ulp_f32(Dn[1]), coef * gbbar + 2 * ulp_f32(dn[1])
    for name, got, ref, bar in (("dW2", dW[2], Dn[1], dWbar), ("W2", W[2], Wn[1], dWbar + 2 * ulp_f32(Wn[1])), ("db2", db[2], dn[1], dbbar),
                                ("b2", b[2], bn[1], dbbar + 2 * ulp_f32(bn[1]))):
        res.checks.append(check(name, f32(got).reshape(ref.shape), ref, bar))
    res.figures.update(rho_ref=rho, rho_ref_bias_sum=rho_b, update_coefficient=coef)
    return res


RUN = {"C": run_C, "F": run_F, "T": run_T, "O": run_O, "E": run_E, "D": run_D, "W": run_W, "U": run_U}


def run_case(c, make):
    """The case on a device: make(ls, B, act, out, W, b) gives an object with forward(x), grads(x, t) -> the padded (gw, gb) of the
    bunch, train(x, t) -> (W, b, dW, db) after one step from zero momentum, and close()."""
    p = problem(c.id)
    dev = make(c.ls, c.B, c.act, c.out, p.W, p.b)
    try:
        return RUN[c.family](c, p, dev, make)
    finally:
        dev.close()


# ------------------------------------------------------------------ the bf16 step in numpy
MUTANTS = collections.OrderedDict([
    ("truncating_store", ("F", "E", "D")), ("ties_away_from_zero", ("C",)), ("bias_after_rounding", ("F",)), ("ct_one_row_off", ("T",)),
    ("act_from_next_row", ("D",)), ("scale_after_rounding", ("E",)), ("k_slab_dropped", ("O", "W"))])


class Model(object):
    """The device's bf16 step: bf16 storage of everything a GEMM reads, fp32 accumulation in `width`-wide k-slabs, ascending or
    (reverse) descending, fp32 epilogues as csrc/bp_bf16.h writes them.  hidden: yb, ybT, dxb, dxbT by name after a call."""

    def __init__(self, ls, B, act, out, W, b, width=16, reverse=False, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.ls, self.B, self.act, self.out, self.L = list(ls), B, act, out, len(ls)
        self.width, self.reverse, self.mutant = width, reverse, mutant
        self.W = [None] + [f32(w).copy() for w in W[1:]]
        self.b = [None] + [f32(v).copy() for v in b[1:]]
        self.Wb = [None] + [self.store(w, convert=True) for w in self.W[1:]]
        self.hidden = {}

    def store(self, v, convert=False):
        u = np.ascontiguousarray(v, np.float32).view(np.uint32)
        if self.mutant == "truncating_store":
            return (u & np.uint32(0xFFFF0000)).view(np.float32)
        if self.mutant == "ties_away_from_zero" and convert:
            return ((u + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(np.float32)
        return bf16_round(v).astype(np.float32)

    def acc(self, A, Bm, droppable=False):
        A, Bm = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(Bm, np.float32)
        K, w = A.shape[1], self.width
        starts = list(range(0, K, w))
        if self.mutant == "k_slab_dropped" and droppable:               # (w divides 16)
            lo = (K // 2) // 16 * 16
            starts = [k0 for k0 in starts if not lo <= k0 < lo + 16]
        z = np.zeros((A.shape[0], Bm.shape[1]), np.float32)
        for k0 in (reversed(starts) if self.reverse else starts):
            z += A[:, k0:k0 + w] @ Bm[k0:k0 + w]
        return z

    def _transposed(self, y):
        return np.roll(y, 1, axis=0) if self.mutant == "ct_one_row_off" else y

    def _forward(self, x):
        L, h = self.L, self.hidden
        h.clear()
        h["yb0"] = h["ybT0"] = self.store(x, convert=True)
        for l in range(1, L - 1):
            z = self.acc(h["yb%d" % (l - 1)], self.Wb[l])
            if self.mutant == "bias_after_rounding":
                z = self.store(z)
            z = z + self.b[l]
            y = np.maximum(z, np.float32(0.0)) if self.act == 0 else sigmoid32(z)
            h["yb%d" % l] = self.store(y)
            h["ybT%d" % l] = self._transposed(h["yb%d" % l])
        z = self.acc(h["yb%d" % (L - 2)], self.Wb[L - 1], droppable=True) + self.b[L - 1]
        if self.out:
            z[:, self.out[0]:] = sigmoid32(z[:, self.out[0]:])
        return z

    def forward(self, x):
        return self._forward(f32(x))

    def _grads(self, x, t):
        L, B, h = self.L, self.B, self.hidden
        o = self._forward(f32(x))
        s = np.float32(2.0) / np.float32(B)
        e = o - f32(t)
        d = s * self.store(e) if self.mutant == "scale_after_rounding" else s * e
        if self.out and self.out[1] == 1:
            lin = self.out[0]
            d[:, lin:] *= o[:, lin:] * (np.float32(1.0) - o[:, lin:])
        h["dxb%d" % (L - 1)] = h["dxbT%d" % (L - 1)] = self.store(d)
        for l in range(L - 1, 1, -1):
            a = self.acc(h["dxb%d" % l], self.Wb[l].T)
            y = h["yb%d" % (l - 1)]
            if self.mutant == "act_from_next_row":
                y = y[np.minimum(np.arange(B) + 1, B - 1)]
            actp = (y > 0).astype(np.float32) if self.act == 0 else (np.float32(1.0) - y) * y
            h["dxb%d" % (l - 1)] = self.store(actp * a)
            h["dxbT%d" % (l - 1)] = self._transposed(h["dxb%d" % (l - 1)])
        dma = D.pad64(B) in (128, 256, 512, 1024)                   # the grouped launch sums the panel it streams: the transposed copy
        gw = [None] + [self.acc(h["ybT%d" % (l - 1)].T, h["dxbT%d" % l], droppable=l == L - 1) for l in range(1, L)]
        gb = [None] + [self.acc(np.ones((1, B), np.float32), h["dxbT%d" % l if dma else "dxb%d" % l])[0] for l in range(1, L)]
        return gw, gb

    def grads(self, x, t):
        gw, gb = self._grads(x, t)
        pw, pb = [None], [None]
        for l in range(1, self.L):
            P, N = D.pad64(self.ls[l - 1]), D.pad64(self.ls[l])
            w, v = np.zeros((P, N), np.float32), np.zeros(N, np.float32)
            w[:self.ls[l - 1], :self.ls[l]], v[:self.ls[l]] = gw[l], gb[l]
            pw.append(w)
            pb.append(v)
        return pw, pb

    def train(self, x, t):
        gw, gb = self._grads(x, t)
        m, c1, n = np.float32(MOM), np.float32((1 - np.float32(MOM)) * np.float32(LR)), np.float32(self.B)
        dW = [None] + [m * np.float32(0.0) - c1 * (gw[l] / n + np.float32(WC) * self.W[l]) for l in range(1, self.L)]
        db = [None] + [m * np.float32(0.0) - c1 * (gb[l] / n) for l in range(1, self.L)]
        W = [None] + [dW[l] + self.W[l] for l in range(1, self.L)]
        b = [None] + [db[l] + self.b[l] for l in range(1, self.L)]
        return W, b, dW, db

    def close(self):
        pass


def model_factory(width=16, reverse=False, mutant=None, keep=None):
    """make() for run_case; keep: a list that receives the models made (the first is the case's own)."""
    def make(ls, B, act, out, W, b):
        m = Model(ls, B, act, out, W, b, width, reverse, mutant)
        if keep is not None:
            keep.append(m)
        return m
    return make


# ------------------------------------------------------------------ the committed figures of a GPU run
GPU_TEST = "tests/test_bf16_iso_gpu.py::test_kernel_alone[%s]"


def numbers(parity):
    """profiles/bf16_iso_parity_numbers.json from the parity JSON of a -m gpu run: one entry per GPU test."""
    tests = {}
    for c in CASES:
        e = parity["tests"].get(GPU_TEST % c.id)
        if e is not None:
            tests[GPU_TEST % c.id] = e["bf16_iso"]
    return {"source": "pytest tests/test_bf16_iso_gpu.py -m gpu on an MI355X; python tests/bf16_iso.py numbers <parity JSON>", "tests": tests}


if __name__ == "__main__":
    import json
    import sys
    if sys.argv[1:2] == ["numbers"]:
        json.dump(numbers(json.load(open(sys.argv[2]))), sys.stdout, indent=1, sort_keys=True)
        print()
    else:
        for c in CASES:
            print("%-26s %s B %-5d %-66s at layer %d: %s" % (c.id, "x".join(str(v) for v in c.ls), c.B, c.kernel[5:].split("(")[0], c.layer,
                                                          "ok" if launch_at(c) == c.kernel else "dispatch gives " + launch_at(c)))
