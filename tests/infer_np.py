"""The row-invariant inference forward (bp_infer.hip, BP_FORWARD_ROWINV) restated for the tests: which kernel and which
decomposition a layer gets (infer_plan, bp_infer.h), the nets the tests use, which named case of tests/test_infer_gpu.py reaches
what, and the exact-arithmetic data of its parity test (the recipe of tests/exact_data.py).  No GPU, nothing from the product."""
import numpy as np

import exact_data as ED

BM, BN, KU, MAX_SPLITK = 32, 128, 16, 8


def pad64(x):
    return (x + 63) // 64 * 64


def plan(K, N):
    """(tiles_n, splitk, per) of a layer with padded widths K -> N: a function of the shape alone."""
    U = K // KU
    tiles_n = (N + BN - 1) // BN
    splitk = 1
    while splitk < MAX_SPLITK and tiles_n * splitk * 2 <= 128 and U // (4 * splitk * 2) >= 3:
        splitk *= 2
    return tiles_n, splitk, (U + 4 * splitk - 1) // (4 * splitk)


def kernel(K, N):
    return "void bp_infer_layer<%s>(InferArgs)" % ("true" if plan(K, N)[1] > 1 else "false")


def layer_claims(K, N, rows, B):
    """The kernel of a layer and the branches of it that a call of `rows` rows on a handle of bunch B takes."""
    tiles_n, splitk, per = plan(K, N)
    U, name = K // KU, kernel(K, N)
    out = {name, "%s | %d k-slices" % (name, splitk)}
    out.add("%s | %s" % (name, "last column tile half empty" if N % BN else "whole column tiles"))
    out.add("%s | %s" % (name, "partial sums without k-rows" if (4 * splitk - 1) * per >= U else
                         "uneven partial sums" if 4 * splitk * per != U else "even partial sums"))
    for fb in set([min(B, rows)] + ([rows % B] if rows > B and rows % B else [])):
        out.add("%s | %s" % (name, "one row tile" if fb <= BM else "several row tiles"))
        out.add("%s | %s" % (name, "row tile ends inside" if fb % BM else "whole row tiles"))
    return out


def claims(ls, rows, B):
    ld = [pad64(s) for s in ls]
    out = set()
    for l in range(1, len(ls)):
        out |= layer_claims(ld[l - 1], ld[l], rows, B)
    # layers with different slice counts share the slab (each at its own stride) and have ticket words of their own
    if len(set(plan(ld[l - 1], ld[l])[1] for l in range(1, len(ls)))) > 1:
        out.add("%s | layers with different slice counts" % kernel(2048, 2048))
    return out


# The nets of tests/test_infer_gpu.py.  S: the net of tests/test_stream_gpu.py (FD 33, context 7 + the noise-aware block): K = 320
# and 128, no multiple of 256, N = 128 and 64 -- no k-slices.  S66: S with the 66-wide output of the mask configuration.
# W: the wide layers, every one of them k-split (8 slices; K = 1600 leaves partial sums without k-rows).
# M: the smallest net with 4, 8 and 2 slices in one net (1024 -> 4096: 32 column tiles allow 4; 4096 -> 576: 8; 576 -> 192: 2, and
# its 36 units over 8 partial sums of 5 leave the last one a single unit: uneven).  The widest layer has the fewest slices, so
# the other layers' slices lie at other strides in the shared slab.
NET_S, NET_S66, NET_W, NET_M = [264, 96, 33], [264, 96, 66], [1548, 2048, 2048, 129], [1000, 4096, 570, 129]
# named case of tests/test_infer_gpu.py -> (layer sizes, rows of its largest call, bunch size)
CASES = {
    "test_invariance[S]": (NET_S, 100, 32),
    "test_invariance[S] second handle": (NET_S, 100, 7),
    "test_invariance[W]": (NET_W, 100, 64),
    "test_invariance[W] second handle": (NET_W, 100, 256),
    "test_invariance[M]": (NET_M, 100, 64),
    "test_invariance[M] second handle": (NET_M, 100, 256),
    "test_parity[S66]": (NET_S66, 65, 32),
    "test_parity[M]": (NET_M, 65, 64),
    "test_exact[M]": (NET_M, 65, 64),
    "test_exact[S]": (NET_S, 65, 32),
    "test_exact[W]": (NET_W, 65, 64),
}


def case_claims():
    return {k: claims(*v) for k, v in CASES.items()}


# ------------------------------------------------------------------ data whose arithmetic is exact (tests/exact_data.py)
def exact_net(ls, seed):
    """Integer weights on weight_pattern (+-1, +-2; the three-weight-layer net W: +-1, its sums would pass 2^24 quanta), biases
    in halves."""
    rng = np.random.default_rng(seed)
    vals = np.array([-1.0, 1.0] if len(ls) > 3 else [-2.0, -1.0, 1.0, 2.0], np.float32)
    W, b = [None], [None]
    for l in range(1, len(ls)):
        nz = ED.weight_pattern(rng, ls[l - 1], ls[l])
        W.append(np.where(nz, rng.choice(vals, size=(ls[l - 1], ls[l])), np.float32(0.0)).astype(np.float32))
        b.append((rng.integers(-2, 3, size=ls[l]) * 0.5).astype(np.float32))
    return W, b


def exact_inputs(ls, n, seed):
    rng = np.random.default_rng(seed + 100)
    return (rng.integers(-3, 4, size=(n, ls[0])) * 0.5).astype(np.float32)


def exact_forward(ls, W, b, x):
    """float64 forward (ReLU, linear output): (out, [(name, A, B, bias)] of every GEMM, live share of every hidden layer)."""
    y, gemms, live = np.asarray(x, np.float64), [], {}
    for l in range(1, len(ls)):
        A, Bm, bias = y, np.asarray(W[l], np.float64), np.asarray(b[l], np.float64)
        gemms.append(("forward %d" % l, A, Bm, bias))
        z = A @ Bm + bias
        if l < len(ls) - 1:
            live[l] = float((z > 0).mean())
            y = np.maximum(z, 0.0)
    return z, gemms, live


def exact_conditions(ls, W, b, x):
    """Failures of conditions (a) and (c) of tests/exact_data.py on the forward GEMMs (an empty list: they hold), and the figures."""
    out, gemms, live = exact_forward(ls, W, b, x)
    fails, fig = [], {"max_over_q_log2": 0.0, "live": live}
    for name, A, Bm, bias in gemms:
        m, q = ED.gemm_bounds(A, Bm, bias)
        fig["max_over_q_log2"] = max(fig["max_over_q_log2"], float(np.log2(max(m / q, 1.0))))
        if not (m / q < 2.0 ** 24 and q >= 2.0 ** -40):
            fails.append("(a) %s: max sum |a||b| = %g, q = 2^%d" % (name, m, int(np.log2(q))))
        holes = ED.slab_holes(A, Bm)
        if holes:
            fails.append("(c) %s: %d (slab, block row, block column) without weight, first %s" % (name, len(holes), holes[:3]))
    for l, v in live.items():
        if not 0.25 <= v <= 0.75:
            fails.append("(c) %.0f %% of the ReLUs of layer %d are live" % (100 * v, l))
    if not np.array_equal(out.astype(np.float32).astype(np.float64), out):
        fails.append("the output is no fp32 number")
    return fails, fig
