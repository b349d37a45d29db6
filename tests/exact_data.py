"""Data on which one training step is exact arithmetic, for the cases of tests/dispatch_cases.py (no GPU, nothing from the product
is imported; tests/test_exact_host.py checks the conditions below on the CPU, tests/test_exact_gpu.py holds the device to them).

The recipe.  W_l: integers in [-2, 2] ([-1, 1] in nets of more than four weight layers), non-zero in one place per row and per
column of every 16 x 16 block and in at least 12 places per column (weight_pattern: no 16-wide slab of a forward or dgrad reduction
is empty in any column, however wide the layer); biases: multiples of 1/2 in [-1, 1]; inputs: multiples of 1/2 in [-1.5, 1.5];
hidden activation ReLU for every case (kernel names do not depend on it: exact_case); lr 0.5, momentum 0.5, no weight cost;
targets t = o_ref - d B/2 with d
drawn from {0, +-1/4, ..., +-1} and o_ref the reference's own output of that bunch.  Then o - t = d B/2 exactly and
bf16(fl32(fl32(2/B) (o - t))) = d for any bunch size B: the bf16 rounding snaps the one-ulp error of 2/B back (fp32 handles need
2/B exact: a power-of-two bunch).  On the logistic columns of a logistic case t = y_ref - d B/2 with d != 0, y_ref = 1/(1 + exp(-o_ref)):
whatever the last bits of the device's expf, (2/B)(y - t) rounds to d and never to a stray tiny number; the oracle, which has only
the linear output, gets the targets o_ref - d B/2 there and so the same dEdX (t_oracle).

Every value that is stored is then a multiple of one power of two q (integer weights keep the quantum through any depth; the bf16
rounding of a multiple of q is a multiple of q), and the step is exact under three conditions, which are conditions on the DATA,
checked from the reference alone:

 (a) exact accumulation.  For every GEMM of the step (each forward, dgrad, weight gradient and bias sum; operands as
     oracle/bp_oracle.c stores them): max sum_k |a||b| / q < 2^24 and q >= 2^-40, q the largest power of two that divides every
     term.  Then every partial sum in every order is an fp32 number: the result does not depend on the summation order, the
     k-split, the tile shape or the accumulator type.  (gemm_bounds)
 (b) the oracle agrees with itself: fp32 and fp64 accumulation give array_equal gradients, outputs and state after one step.
 (c) the data can see a defect.  Every 16-wide slab of the reduction dimension of every GEMM contributes a non-zero to every
     64 x 64 block of that GEMM's output (slab_holes; the bias sums: to every 64-column tile); 25 .. 75 % of the ReLUs of every
     hidden layer are live; every G_l has more than 256 distinct values and no all-zero 64 x 64 block.

A shard problem (SHARD_CASES) is the same at a global bunch Bg = 2B and a rank_frame_offset: t = o_ref - d Bg/2, and the masks are
those of the global frames from the offset on.

What it cannot cover: a second step (the updated weights are no longer few-bit numbers), Sigmoid nets, logistic forward columns.
Nor any bf16 store that rounds: tests/bf16_iso.py is the partner for that, each kernel alone on generic operands at half-ulp bars."""
import numpy as np

import dispatch_cases as DC
import dispatch_np as D
from torch_ref import bf16_round

LR, MOM, WC = 0.5, 0.5, 0.0
DROP = dict(dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=77)
D_VALUES = np.array([0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0, -1.0])
CV_ERRORS = np.array([0.0, 1.0, -1.0, 2.0, -2.0])        # o - t of the CV targets: sums of squares that stay integers below 2^24

BF16_CASES = [c for c in DC.CASES if c.dtype == 1]
FP32_STEP_CASES = ["f32_wide128", "f32_nine_layers_b128", "f32_b512"]     # power-of-two bunches: 2/B is an fp32 number
DROPOUT_CASES = ["bf_rows128", "bf_nine_layers", "bf_rows64"]
# Shard handles (one rank's share of a data-parallel bunch; gradient store only, a shard handle trains through its group): the
# case's bunch B at global bunch 2B and rank_frame_offset 3, with dropout.  dEdX_L = fl32(2/Bg)(o - t), so the targets are
# o_ref - d Bg/2, and the masks are those of the global frames 3 .. B + 2: the last of the two-block branches of drop_words4.
SHARD_CASES = ["bf_rows64", "bf_rows128"]
SHARD_OFFSET = 3


def shard_of(cid):
    """(rank_frame_offset, global bunch) of a shard problem."""
    return SHARD_OFFSET, 2 * DC.BY_ID[cid].B


def exact_case(c):
    """The case as the exact tests run it: ReLU.  The kernels are those of the table's case."""
    e = c._replace(act=0)
    assert D.case_kernels(e.ls, e.B, e.dtype, 1 if e.out else 0) == D.case_kernels(c.ls, c.B, c.dtype, 1 if c.out else 0), c.id
    return e


def _seed(c):
    """One seed per case.  Most of (c) holds by construction (weight_pattern); what the seed decides is whether a sum over 16 frames
    or 16 units cancels to zero in a ragged edge block one or two columns wide -- tests/test_exact_host.py says whether it does."""
    return [k.id for k in DC.CASES].index(c.id)


def weight_values(c):
    """Integers in [-2, 2]; nets of more than four weight layers: [-1, 1].  The activations of this data grow by about
    sqrt(k E[w^2] / 2) per layer; with +-2 the eight-layer net's weight-gradient sums pass 2^24 quanta (condition (a))."""
    return np.array([-1.0, 1.0] if len(c.ls) - 1 > 4 else [-2.0, -1.0, 1.0, 2.0], np.float32)


def weight_pattern(rng, prev, cur):
    """Where W_l is non-zero: in every 16 x 16 block one element per row and per column (a shuffled diagonal; a ragged edge block
    r x c wraps it), so that every column meets every 16-row slab of the forward and every row every 16-column slab of the dgrad;
    then columns with fewer than 12 non-zeros are filled up to 12."""
    nz = np.zeros((prev, cur), bool)
    for i0 in range(0, prev, 16):
        r = min(16, prev - i0)
        for j0 in range(0, cur, 16):
            cc = min(16, cur - j0)
            m = max(r, cc)
            nz[i0 + np.arange(m) % r, j0 + rng.permutation(m) % cc] = True
    k = min(prev, 12)
    for j in np.flatnonzero(nz.sum(0) < k):
        free = np.flatnonzero(~nz[:, j])
        nz[rng.choice(free, size=k - (prev - free.size), replace=False), j] = True
    return nz


def net(c):
    """W[l] ([prev][cur]) and b[l], l = 1 .. L-1 (index 0 unused), fp32."""
    rng = np.random.default_rng(_seed(c))
    vals = weight_values(c)
    W, b = [None], [None]
    for l in range(1, len(c.ls)):
        prev, cur = c.ls[l - 1], c.ls[l]
        nz = weight_pattern(rng, prev, cur)
        W.append(np.where(nz, rng.choice(vals, size=(prev, cur)), np.float32(0.0)).astype(np.float32))
        b.append((rng.integers(-2, 3, size=cur) * 0.5).astype(np.float32))
    return W, b


def inputs(c, n):
    """n frames; a longer chunk starts with the frames of a shorter one."""
    rng = np.random.default_rng(_seed(c) + 100)
    return (rng.integers(-3, 4, size=(n, c.ls[0])) * 0.5).astype(np.float32)


def oracle(c, W, b, acc_double=False, drop=False):
    from oracle import oracle as O
    return O.Oracle(c.ls, c.B, LR, MOM, WC, W, b, activation=0, compute_dtype=c.dtype, acc_double=acc_double, **(DROP if drop else {}))


def masks(c, W, b, gframe0=0):
    """The Philox masks of the first step of a handle (step 0, frames counted from the start of the bunch, which is global frame
    gframe0), as the oracle draws them."""
    o = oracle(c, W, b, drop=True)
    return [o.fill_mask(0, l, c.B, gframe0=gframe0) for l in range(len(c.ls) - 1)]


def reference_outputs(c, W, b, x, drop=False, gframe0=0):
    """The pre-activation output of every frame: training mode (with the masks of `masks`) for the whole bunches when drop, else the
    plain forward."""
    o = oracle(c, W, b)
    if not drop:
        return o.forward(x)
    mk, B = masks(c, W, b, gframe0), c.B
    out = o.forward(x)                                             # (the trailing partial bunch is never trained on)
    for i in range(x.shape[0] // B):
        out[i * B:(i + 1) * B] = o.grads(x[i * B:(i + 1) * B], np.zeros((B, c.ls[-1]), np.float32), masks=mk)[3]
    return out


def train_targets(c, W, b, x, drop=False, shard=None):
    """(t, t_oracle, d): the targets of the handle, those of the oracle (they differ on logistic columns only) and the dEdX_L both
    must arrive at, [n][sL] each.  The rows of a longer chunk start with those of a shorter one.  shard = (offset, Bg): the scale
    is 2/Bg, the masks those of the global frames from offset on."""
    n, sL, B = x.shape[0], c.ls[-1], (c.B if shard is None else shard[1])
    rng = np.random.default_rng(_seed(c) + 200 + (50 if drop else 0) + (7 if shard else 0))
    o = reference_outputs(c, W, b, x, drop, shard[0] if shard else 0).astype(np.float64)
    idx = rng.integers(0, len(D_VALUES), size=(n, sL))
    if c.out is not None:
        lin = c.out[0]
        assert c.out[1] == 0, "loss 0 only: with the squared error through the logistic dEdX is not d"
        idx[:, lin:] = idx[:, lin:] % (len(D_VALUES) - 1) + 1                              # d != 0
    d = D_VALUES[idx]
    t_oracle = o - d * (B / 2.0)
    assert np.array_equal(t_oracle.astype(np.float32).astype(np.float64), t_oracle), (c.id, "the targets are no fp32 numbers")
    t = t_oracle.copy()
    if c.out is not None:
        with np.errstate(over="ignore"):
            y = (np.float32(1.0) / (np.float32(1.0) + np.exp(-o[:, lin:].astype(np.float32)))).astype(np.float64)
        t[:, lin:] = y - d[:, lin:] * (B / 2.0)
    return t.astype(np.float32), t_oracle.astype(np.float32), d


def cv_targets(c, W, b, x):
    """Targets with o - t in {0, +-1, +-2} on the linear columns: the sum of squares is a small integer.  On logistic columns the
    error is not exact whatever the target (None is returned for the sum there)."""
    rng = np.random.default_rng(_seed(c) + 300)
    o = reference_outputs(c, W, b, x).astype(np.float64)
    e = CV_ERRORS[rng.integers(0, len(CV_ERRORS), size=o.shape)]
    t = (o - e).astype(np.float32)
    assert np.array_equal(t.astype(np.float64), o - e), c.id
    if c.out is not None:
        t[:, c.out[0]:] = (rng.random((x.shape[0], c.ls[-1] - c.out[0])) < 0.4).astype(np.float32)
        return t, None, "logistic columns: the squared error of 1/(1 + exp(-z)) is not exact on any data"
    total, q = float((e * e).sum()), 1.0
    if not total / q < 2.0 ** 24:
        return t, None, "sum of squares %.0f is no fp32 partial sum in every order" % total
    return t, total, None


# ------------------------------------------------------------------ the step restated, operands kept
def quantum(*arrays):
    """The largest power of two that divides every value of the arrays (1.0 for all-zero arrays)."""
    v = np.concatenate([np.abs(np.asarray(a, np.float64)).ravel() for a in arrays])
    v = v[v != 0]
    if v.size == 0:
        return 1.0
    m, e = np.frexp(v)                                             # v = m 2^e, 0.5 <= m < 1: m 2^53 is an integer
    i = np.ldexp(m, 53).astype(np.int64)
    low = np.log2((i & -i).astype(np.float64)).astype(np.int64)    # its trailing zero bits
    return float(2.0 ** int((e - 53 + low).min()))


class Bunch(object):
    """One bunch in float64 with the storage rounding of oracle/bp_oracle.c (compute_dtype 1: weights, the masked input, every hidden
    output and every dEdX_l are bf16 numbers).  gemms: (name, A [M][K], B [K][N], addend [N] or None) of every GEMM of the step."""

    def __init__(self, c, W, b, x, t, mk=None, Bg=None):
        L, B = len(c.ls), x.shape[0]
        r = bf16_round if c.dtype == 1 else (lambda v: np.asarray(v, np.float64))
        Wb = [None] + [r(W[l]) for l in range(1, L)]
        h = np.asarray(x, np.float64)
        ys, self.live, self.gemms = [r(h * (1.0 - mk[0]) if mk else h)], {}, []
        for l in range(1, L):
            bias = np.asarray(b[l], np.float64)
            z = ys[l - 1] @ Wb[l] + bias
            self.gemms.append(("forward %d" % l, ys[l - 1], Wb[l], bias))
            if l < L - 1:
                self.live[l] = float((z > 0).mean())
                y = np.maximum(z, 0.0)
                ys.append(r(y * (1.0 - mk[l]) if mk else y))
        self.out = z
        s = np.float32(2.0) / np.float32(Bg or B)                                          # kernSubClean, in fp32 as both sides do it
        dx = {L - 1: r((s * (z.astype(np.float32) - np.asarray(t, np.float32))).astype(np.float32))}
        assert np.array_equal(z.astype(np.float32).astype(np.float64), z), (c.id, "the output is no fp32 number")
        for l in range(L - 1, 1, -1):
            self.gemms.append(("dgrad %d" % l, dx[l], Wb[l].T, None))
            dx[l - 1] = r((ys[l - 1] > 0) * (dx[l] @ Wb[l].T))
        self.ys, self.dx = ys, dx
        self.gw, self.gb = [None], [None]
        for l in range(1, L):
            self.gemms.append(("wgrad %d" % l, ys[l - 1].T, dx[l], None))
            self.gemms.append(("bias sum %d" % l, np.ones((1, B)), dx[l], None))
            self.gw.append(ys[l - 1].T @ dx[l])
            self.gb.append(dx[l].sum(0))


def gemm_bounds(A, Bm, addend=None):
    """(max sum_k |a||b| (+ |addend|), q): condition (a) asks max / q < 2^24 and q >= 2^-40."""
    m = np.abs(A) @ np.abs(Bm)
    q = quantum(A) * quantum(Bm)
    if addend is not None:
        m = m + np.abs(addend)
        q = min(q, quantum(addend))
    return float(m.max()), q


def slab_holes(A, Bm, slab=16, block_rows=64):
    """Condition (c): the (slab, block row, block column) triples whose slab of the reduction dimension contributes nothing but
    zeros to that block_rows x 64 block of A . B (an empty list is what the condition asks).  fp32 products: exact under (a)."""
    M, K = A.shape
    N = Bm.shape[1]
    br = M if block_rows is None else block_rows
    Mp, Np = -(-M // br) * br, -(-N // 64) * 64
    A32, B32 = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(Bm, np.float32)
    P = np.zeros((Mp, Np), np.float32)
    holes = []
    for k0 in range(0, K, slab):
        np.matmul(A32[:, k0:k0 + slab], B32[k0:k0 + slab], out=P[:M, :N])
        hit = (P != 0).reshape(Mp // br, br, Np // 64, 64).any(axis=(1, 3))
        holes += [(k0 // slab, int(i), int(j)) for i, j in np.argwhere(~hit)]
    return holes


def zero_blocks(G):
    """The 64 x 64 blocks of G (true extent) that hold nothing but zeros."""
    M, N = G.shape
    return [(i, j) for i in range(0, M, 64) for j in range(0, N, 64) if not G[i:i + 64, j:j + 64].any()]


# ------------------------------------------------------------------ comparing bit for bit
def unequal(name, got, ref):
    """None when the two are array_equal; else the failure text: the tensor, the worst 64 x 64 block (in the style of
    test_dispatch_gpu.worst_block), how many elements differ, what size the error has, and the first unequal pair as hex words."""
    a, r = np.atleast_2d(np.asarray(got, np.float32)), np.atleast_2d(np.asarray(ref, np.float32))
    assert a.shape == r.shape, (name, a.shape, r.shape)
    if np.array_equal(a, r):
        return None
    ne = a != r
    d = np.abs(a.astype(np.float64) - r.astype(np.float64))
    d[~np.isfinite(d)] = np.inf
    i, j = np.unravel_index(int(d.argmax()), d.shape)
    i0, j0 = (i // 64) * 64, (j // 64) * 64
    blocks = sorted(set((int(p) // 64 * 64, int(q) // 64 * 64) for p, q in np.argwhere(ne)))
    fi, fj = np.argwhere(ne)[0]
    ulps = d[ne] / np.spacing(np.maximum(np.abs(a[ne]), np.abs(r[ne]))).astype(np.float64)   # (unequal: the larger one is not 0)
    return ("%s: %d of %d elements unequal in %d blocks of 64 x 64 (first blocks %s); worst block rows %d.., cols %d.. (of %s): "
            "max|err| %.9g at [%d, %d] (ref %.9g), %d unequal in that block; errors between %.3g and %.3g fp32 ulps of the larger of the pair; "
            "first unequal [%d, %d]: got 0x%08x, ref 0x%08x"
            % (name, int(ne.sum()), ne.size, len(blocks), blocks[:4], i0, j0, a.shape, d[i, j], i, j, r[i, j],
               int(ne[i0:i0 + 64, j0:j0 + 64].sum()), ulps.min(), ulps.max(), fi, fj, int(a[fi, fj].view(np.uint32)), int(r[fi, fj].view(np.uint32))))


def count_unequal(got, ref):
    return int((np.asarray(got, np.float32) != np.asarray(ref, np.float32)).sum())


def within_one_ulp(got, ref):
    """Every element equal or one fp32 ulp of the reference away."""
    a, r = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - r.astype(np.float64)) <= np.spacing(np.abs(r)).astype(np.float64)))


# ------------------------------------------------------------------ what the tests of a case share
class _Bag(object):
    pass


def _frozen(a):
    if isinstance(a, np.ndarray):
        a.setflags(write=False)
    elif isinstance(a, (list, tuple)):
        for v in a:
            _frozen(v)
    return a


_PROBLEMS, _REFERENCES = {}, {}


def steps_exactly(c):
    """Whether the gradient and the fused step of the case are held exactly (every bf16 case; fp32: power-of-two bunches)."""
    return c.dtype == 1 or c.id in FP32_STEP_CASES


def problem(cid, drop=False, shard=None):
    """The data of a case, made once and read-only: c (exact_case), W, b, x (2B + B/2 frames: two whole bunches and a partial one),
    t (the handle's training targets), t_oracle, d, masks (drop: the step-0 Philox masks, else None), t_cv, cv_sum, cv_skip.
    shard: shard_of(cid) for the shard problem of the case (always with dropout)."""
    if (cid, drop, shard) not in _PROBLEMS:
        p = _Bag()
        p.c = c = exact_case(DC.BY_ID[cid])
        p.W, p.b = net(c)
        p.x = inputs(c, 2 * c.B + c.B // 2)
        p.shard = shard
        p.t, p.t_oracle, p.d = train_targets(c, p.W, p.b, p.x, drop, shard)
        p.masks = masks(c, p.W, p.b, shard[0] if shard else 0) if drop else None
        p.t_cv, p.cv_sum, p.cv_skip = cv_targets(c, p.W, p.b, p.x)
        _frozen([p.W[1:], p.b[1:], p.x, p.t, p.t_oracle, p.d, p.masks, p.t_cv])
        _PROBLEMS[(cid, drop, shard)] = p
    return _PROBLEMS[(cid, drop, shard)]


def reference(cid, drop=False, acc_double=False, shard=None):
    """The oracle's results on problem(cid, drop), computed once and read-only: grads[k] = (gw, gb) of bunch k = 0, 1; state =
    (W, b, dW, db) after one step on bunch 0 from zero momentum; forward = the output of the first B + 3 frames; cv = CrossValid
    on the whole chunk against t_cv.  acc_double (the oracle's slow loops, condition (b) only): bunch 0, state and forward.
    shard: the gradients at scale 2/Bg; the state is that of the update on bunch 0's gradient, which no shard handle performs."""
    key = (cid, drop, acc_double, shard)
    if key not in _REFERENCES:
        p, r = problem(cid, drop, shard), _Bag()
        c, B = p.c, p.c.B
        o = oracle(c, p.W, p.b, acc_double, drop)
        r.grads = [o.grads(p.x[k * B:(k + 1) * B], p.t_oracle[k * B:(k + 1) * B], masks=p.masks, scale_frames=shard[1] if shard else None)[:2]
                   for k in ((0,) if acc_double else (0, 1))]
        r.forward = oracle(c, p.W, p.b, acc_double).forward(p.x[:B + 3])
        r.cv = oracle(c, p.W, p.b).crossvalid(p.x, p.t_cv) if p.cv_sum is not None and not acc_double else None
        o.update(r.grads[0][0], r.grads[0][1], B)                  # one step from zero momentum = the update on bunch 0's gradient
        r.state = (o.W, o.b, o.dW, o.db)
        _frozen([[g[0][1:], g[1][1:]] for g in r.grads] + [r.forward] + [s[1:] for s in r.state])
        _REFERENCES[key] = r
    return _REFERENCES[key]


def conditions(cid, drop=False, shard=None):
    """(failures, figures) of the conditions (a) - (c) on problem(cid, drop): a list of texts, empty when all hold, and what was
    measured.  A case that is held on the forward and CV only (an fp32 bunch that is no power of two) is asked about its forward
    GEMMs only."""
    p = problem(cid, drop, shard)
    c, B, L = p.c, p.c.B, len(p.c.ls)
    step = steps_exactly(c)
    fails, fig = [], {"max_over_q_log2": 0.0, "q_min_log2": 0, "live": {}, "distinct": {}}
    for k in (0, 1):
        sl = slice(k * B, (k + 1) * B)
        bu = Bunch(c, p.W, p.b, p.x[sl], p.t_oracle[sl], p.masks, shard[1] if shard else None)
        if step and not np.array_equal(bu.dx[L - 1], p.d[sl]):
            fails.append("bunch %d: dEdX_L is not d in %d places" % (k, int((bu.dx[L - 1] != p.d[sl]).sum())))
        for name, A, Bm, add in bu.gemms:
            if not step and not name.startswith("forward"):
                continue
            m, q = gemm_bounds(A, Bm, add)
            fig["max_over_q_log2"] = max(fig["max_over_q_log2"], float(np.log2(max(m / q, 1.0))))
            fig["q_min_log2"] = min(fig["q_min_log2"], int(np.log2(q)))
            if not (m / q < 2.0 ** 24 and q >= 2.0 ** -40):
                fails.append("(a) bunch %d %s: max sum |a||b| = %g, q = 2^%d" % (k, name, m, int(np.log2(q))))
            holes = slab_holes(A, Bm, block_rows=None if A.shape[0] == 1 else 64)
            if holes:
                fails.append("(c) bunch %d %s: %d (slab, block row, block column) without weight, first %s" % (k, name, len(holes), holes[:3]))
        for l, v in bu.live.items():
            fig["live"]["bunch %d layer %d" % (k, l)] = v
            if not 0.25 <= v <= 0.75:
                fails.append("(c) bunch %d: %.0f %% of the ReLUs of layer %d are live" % (k, 100 * v, l))
        if not step:
            continue
        for l in range(1, L):
            n = int(np.unique(bu.gw[l]).size)
            fig["distinct"]["bunch %d G%d" % (k, l)] = n
            if not n > 256:
                fails.append("(c) bunch %d: G%d has %d distinct values" % (k, l, n))
            if zero_blocks(bu.gw[l]):
                fails.append("(c) bunch %d: G%d has all-zero blocks %s" % (k, l, zero_blocks(bu.gw[l])[:3]))
        # (b), and the restatement above is the oracle's arithmetic
        r32, r64 = reference(cid, drop, shard=shard), reference(cid, drop, acc_double=True, shard=shard)
        for l in range(1, L):
            for name, i, mine in (("G%d" % l, 0, bu.gw[l]), ("gb%d" % l, 1, bu.gb[l])):
                a = r32.grads[k][i][l]
                r = r64.grads[k][i][l] if k == 0 else a
                if not np.array_equal(a, r):
                    fails.append("(b) bunch %d %s: the oracle's fp32 and fp64 accumulation differ; %s" % (k, name, unequal(name, a, r)))
                if not np.array_equal(a, mine.astype(np.float32)) or not np.array_equal(mine.astype(np.float32).astype(np.float64), mine):
                    fails.append("bunch %d %s: the float64 restatement is not the oracle's gradient" % (k, name))
    r32, r64 = reference(cid, drop, shard=shard), reference(cid, drop, acc_double=True, shard=shard)
    if not np.array_equal(r32.forward, r64.forward):
        fails.append("(b) forward: " + unequal("forward", r32.forward, r64.forward))
    if p.cv_sum is not None and r32.cv != p.cv_sum:
        fails.append("CV sum: the oracle's %r, exact %r" % (r32.cv, p.cv_sum))
    if step:
        for i, nm in enumerate(("W", "b", "dW", "db")):
            for l in range(1, L):
                if not np.array_equal(r32.state[i][l], r64.state[i][l]):
                    fails.append("(b) after one step: " + unequal("%s%d" % (nm, l), r32.state[i][l], r64.state[i][l]))
    return fails, fig


def exact_runs():
    """(case id, drop) of everything tests/test_exact_gpu.py runs."""
    return [(c.id, False) for c in DC.CASES] + [(cid, True) for cid in DROPOUT_CASES]

