"""The case table of the dispatch matrix (tests/test_dispatch_gpu.py runs it on the GPU, tests/test_dispatch_coverage.py checks
without one that it claims every kernel).  Each case is a small net whose shape takes the step through kernels, tile-map branches
or grouped launches that no other case reaches; tests/dispatch_np.py says which.

act: hidden activation, 0 ReLU, 1 Sigmoid (every net with a hidden layer of 1024 units or more, or nine layers, uses Sigmoid: no
ReLU decision near zero blurs a plain comparison).  out: None for the linear output, else (linear_cols, loss) of the logistic one.
spread: the CPU oracle's own disagreement on the one-bunch gradient of the case between fp32 accumulation and acc_double=True,
max over the tensors (fp32 cases: max|a - b| / max|b|; bf16 cases: rms), measured with tools in this file (`python
tests/dispatch_cases.py`); None where the oracle has no such output layer.  fp32 cases assert the one-bunch gradient and the
layer outputs at 1e-5 where 4 x spread < 1e-5, else at 1e-4 (strict_bar); bf16 cases deeper than three weight layers or wider
than 2048 add 1.5 x spread to the 2e-2 rms bar."""
import collections

Case = collections.namedtuple("Case", ["id", "ls", "B", "dtype", "act", "out", "spread", "why"])

NINE = [50, 96, 80, 72, 130, 64, 100, 90, 33]

CASES = [
    # ---- fp32
    Case("f32_xcd_narrow", [100, 256, 512, 200], 80, 0, 0, None, 4.76e-07,
         "n-tile counts 8 and 16: the per-XCD tile map of the 32x32 forward, the narrow dgrad and both generic weight-gradient tiles"),
    Case("f32_wide_hidden", [130, 1000, 520, 40], 100, 0, 1, None, 5.67e-07,
         "32x64 forward with 16 and 9 n-tiles, 64-deep wide dgrad with 9 and 16; nothing a multiple of 64, bunch 100"),
    Case("f32_wide128", [72, 600, 1000, 1000, 257], 256, 0, 1, None, 6.98e-07,
         "128-deep wide dgrad with 16 and 10 n-tiles, split output layer, LDS-DMA weight gradient at bunch 256"),
    Case("f32_wide128_ragged", [72, 600, 1000, 257], 100, 0, 1, None, 8.67e-07,
         "128-deep wide dgrad and the split output layer at a bunch of 100 and widths that end inside a tile"),
    Case("f32_out514_linear", [120, 300, 514], 80, 0, 0, None, 4.93e-07,
         "output layer of 514 columns (576 padded, 9 n-tiles of 64), linear, ragged bunch"),
    Case("f32_out514_logistic", [120, 300, 514], 80, 0, 0, (257, 0), None,
         "the same with 257 linear + 257 logistic columns: lin_cols falls inside a tile"),
    Case("f32_logistic_narrow", [64, 96, 33], 32, 0, 0, (16, 0), None, "narrow logistic output layer, unsplit"),
    Case("f32_logistic_split", [100, 1024, 257], 80, 0, 1, (129, 0), None, "logistic output layer on the split launch"),
    Case("f32_nine_layers", NINE, 40, 0, 1, None, 3.56e-07, "eight weight layers: the second group of four of the generic weight gradients"),
    Case("f32_nine_layers_b128", NINE, 128, 0, 1, None, 4.39e-07, "the same through the LDS-DMA weight gradient at bunch 128, fused and store"),
    Case("f32_b512", [100, 130, 60], 512, 0, 0, None, 6.89e-07, "LDS-DMA weight gradient at bunch 512, fused and store"),
    # ---- bf16
    Case("bf_logistic_small", [64, 96, 33], 32, 1, 0, (16, 0), None, "32-row logistic output tile, unsplit"),
    Case("bf_out_split", [100, 1024, 100], 120, 1, 1, None, 7.19e-08, "split-k output forward; padded bunch 128: LDS-DMA weight gradients"),
    Case("bf_out_split_logistic", [100, 1024, 100], 1000, 1, 1, (50, 0), None, "split-k logistic output forward (64 tiles x 4 slices)"),
    Case("bf_rows64", [130, 6600, 40], 300, 1, 1, None, 8.63e-05,
         "64-row forward and dgrad tiles (padded bunch 320, 104 n-tiles), unsplit 32-row output; nothing a multiple of 64"),
    Case("bf_wgrad64", [2100, 1000, 40], 48, 1, 1, None, 1.56e-04, "64-row generic weight gradient (2112 x 1024), update and store"),
    Case("bf_wgrad128", [2048, 1000, 40], 48, 1, 1, None, 1.83e-06, "128-row generic weight gradient (2048 x 1024), update and store"),
    Case("bf_rows128", [70, 2100, 2000, 40], 1000, 1, 1, None, 1.77e-04,
         "128-row forward and dgrad with 33 n-tiles (register-staged) and 32 (LDS-DMA); padded bunch 1024; nothing a multiple of 64"),
    Case("bf_out64", [70, 130, 2000], 1040, 1, 0, None, 1.39e-05, "64-row output tile (padded bunch 1088); 32-row hidden forward, dgrad and weight gradients"),
    Case("bf_out64_logistic", [70, 130, 2000], 1040, 1, 0, (1000, 0), None, "64-row logistic output tile"),
    Case("bf_out128", [70, 130, 2000], 1000, 1, 0, None, 1.71e-05, "128-row output tile (padded bunch 1024)"),
    Case("bf_out128_logistic", [70, 130, 2000], 1000, 1, 0, (1000, 0), None, "128-row logistic output tile"),
    Case("bf_nine_layers", NINE, 200, 1, 1, None, 1.78e-04, "eight weight layers in one grouped LDS-DMA launch at padded bunch 256, fused and store"),
    Case("bf_b512", [70, 130, 64, 20], 500, 1, 0, None, 1.88e-07, "LDS-DMA weight gradients at padded bunch 512, fused and store"),
]
BY_ID = {c.id: c for c in CASES}

# The seven logistic cases once more with the squared error through the logistic (output_loss 1: d *= o (1 - o) on the logistic
# columns).  A list of its own: the kernels are those of the cases above (the loss is a run-time switch), so these claim nothing in
# tests/test_dispatch_coverage.py; tests/switch_cases.py counts them.
LOSS1_CASES = [c._replace(id=c.id + "_mse", out=(c.out[0], 1)) for c in CASES if c.out is not None]

# The handle of the keep-scaled forward and CV pass (tests/test_dispatch_gpu.py::test_forward_and_cv_keep_scaled): it never trains,
# so the dropout keywords only set alpha = 1 - omit in every forward epilogue.
KEEP_DROP = dict(dropoutflag=1, visible_omit=0.1, hid_omit=0.2)


def keep_scales(c, drop=KEEP_DROP):
    """[None, 1 - visible_omit, 1 - hid_omit, ...]: the factor on the product of weight layer l = 1 .. L-1."""
    return [None, 1.0 - drop["visible_omit"]] + [1.0 - drop["hid_omit"]] * (len(c.ls) - 2)


def strict_bar(spread):
    """fp32: the one-bunch gradient holds 1e-5 where the reference alone supports it.  The spread is one sample of what another
    summation order does and the device uses a third; 4 x leaves headroom for the maximum over a larger tensor."""
    return spread is not None and 4.0 * spread < 1e-5


def deep_or_wide(c):
    """bf16: deeper or wider than the nets of test_bf16_step_matches_bf16_oracle (three weight layers, 2048 units)."""
    return len(c.ls) - 1 > 3 or max(c.ls) > 2048


def case_data(c, n_frames):
    """Weights, biases, inputs and targets of a case (seeded)."""
    import numpy as np
    from oracle import bp_numpy as N
    W, _ = N.glorot_net(c.ls, seed=5, beta=1.0)
    rng = np.random.default_rng(17)
    b = [None] + [rng.normal(size=c.ls[l]).astype(np.float32) * 0.1 for l in range(1, len(c.ls))]
    x = rng.normal(size=(n_frames, c.ls[0])).astype(np.float32)
    t = rng.normal(size=(n_frames, c.ls[-1])).astype(np.float32)
    if c.out is not None:                                      # [real-valued | binary mask] targets, the multi-objective layout
        lin = c.out[0]
        t[:, lin:] = (rng.random((n_frames, c.ls[-1] - lin)) < 0.4).astype(np.float32)
    return W, b, x, t


def oracle_spread(c):
    """The spread of the docstring, computed on the CPU; None for a logistic case."""
    import numpy as np
    from oracle import oracle as O
    if c.out is not None:
        return None
    W, b, x, t = case_data(c, c.B)
    kw = dict(activation=c.act, compute_dtype=c.dtype)
    a = O.Oracle(c.ls, c.B, 1.0, 0.5, 0.0, W, b, **kw).grads(x, t)
    d = O.Oracle(c.ls, c.B, 1.0, 0.5, 0.0, W, b, acc_double=True, **kw).grads(x, t)
    worst = 0.0
    for l in range(1, len(c.ls)):
        for p, q in ((a[0][l], d[0][l]), (a[1][l], d[1][l])):
            p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
            if c.dtype == 0:
                e = np.abs(p - q).max() / max(np.abs(q).max(), 1e-30)
            else:
                e = np.sqrt(((p - q) ** 2).sum()) / max(np.sqrt((q ** 2).sum()), 1e-30)
            worst = max(worst, float(e))
    return worst


def markdown_table():
    """The table "case -> kernels" of DESIGN.md 2, from the restatement: for every case the kernels no EARLIER row names."""
    import dispatch_np as D
    rows, seen = ["| case | net, bunch | kernels the case adds |", "|---|---|---|"], set()
    for c in CASES:
        ks = sorted(D.case_kernels(c.ls, c.B, c.dtype, 1 if c.out else 0))
        new = [k for k in ks if k not in seen]
        seen.update(ks)
        short = ", ".join("`%s`" % k[5:k.rindex("(")].replace("GemmKernel", "K") for k in new) or "(tile-map branch / edge tiles only)"
        net = "x".join(str(v) for v in c.ls) if c.ls is not NINE else "nine layers " + "x".join(str(v) for v in c.ls)
        rows.append("| `%s` | %s %s%s, B %d | %s |" % (c.id, "bf16" if c.dtype else "fp32", net, " logistic" if c.out else "", c.B, short))
    return "\n".join(rows)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["table"]:
        print(markdown_table())
    else:
        for c in CASES:
            print("%-24s spread %s" % (c.id, oracle_spread(c)))
