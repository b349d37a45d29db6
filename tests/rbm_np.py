"""One CD-1 step of a restricted Boltzmann machine (the bp_rbm_* block of include/bp_c_api.h), restated in float64, with the data,
the stacks, the hyper sets and the checks that tests/test_rbm_host.py (no GPU) and tests/test_rbm_gpu.py share.

The checks hold every stage of a step to float64 on the operands the implementation under test itself produced (its v0, its s0,
its v1 ...), so that a sample decided within rounding of u never enters a comparison:
  GEMM outputs (p0, v1, p1)   1e-4 of max|expected|                      (the bar of tests/test_infer_gpu.py)
  gW                          1e-4 of max|v0^T p0|: gW is a difference of two such products, so the bar is taken on the positive one
  gc, ga                      1e-4 of max_j sum_r p0 and of max_i sum_r |v0|: the sums of magnitudes their rounding scales with
  recon                       1e-9 relative: double rounding over <= 1e5 terms stays below that
  update                      1e-5 of max|expected| per tensor           (update_cases.BAR)
MUTANTS are nine wrong implementations; miss(name) computes, from this restatement alone, by how many bars the check named in
CAUGHT_BY misses each of them."""
import collections

import numpy as np

import philox_np as P

GEMM_BAR, UPDATE_BAR, RECON_BAR, TEN_STEP_BAR = 1e-4, 1e-5, 1e-9, 1e-4
MUTANT_FACTOR = 10.0

Stack = collections.namedtuple("Stack", ["id", "sizes", "bunch"])
STACKS = collections.OrderedDict((s.id, s) for s in (
    Stack("S", (70, 33, 20), 24),            # no width or bunch a multiple of any tile; one tile per GEMM
    Stack("W", (264, 200, 136), 64),         # several tiles in m and n; layer 2 is Bernoulli
    Stack("K", (520, 300), 128),             # several k-tiles; K = 2 B = 256 in the statistics GEMM
    Stack("S40", (70, 33, 20), 40),          # rows past the bunch inside a 64-row tile
))
N_BUNCHES = 12
Hyper = collections.namedtuple("Hyper", ["lrate", "momentum", "weightcost"])
HYPER = {"A": Hyper(0.002, 0.5, 1.0 / 16), "B": Hyper(0.05, 0.9, 1.0 / 64)}
SEED = 12345


def sig(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def pad64(n):
    return (n + 63) // 64 * 64


def uniforms(seed, step, layer, B, H):
    """u[r][j] of the definition, fp32: word r & 3 of the block keyed by ((r >> 2) H + j, layer, step), >> 8, times 2^-24."""
    r = np.arange(B, dtype=np.uint64)[:, None]
    idx = (r >> np.uint64(2)) * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :]
    w = P.philox4x32_10(idx & P.MASK32, idx >> np.uint64(32), np.full(idx.shape, layer, np.uint64), np.full(idx.shape, step, np.uint64),
                        seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    sel = (r & np.uint64(3)).astype(np.int64) + np.zeros(idx.shape, np.int64)
    word = np.choose(sel, w)
    return (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def rows(stack, bernoulli=False):
    """N_BUNCHES bunches from a teacher: 8 Bernoulli(1/2) latents through a random [8][V] map plus 0.3 N(0,1), standardised per
    column; bernoulli: the sigma of that."""
    V = stack.sizes[0]
    rng = np.random.default_rng(1000 * V + stack.bunch)
    n = N_BUNCHES * stack.bunch
    z = (rng.random((n, 8)) < 0.5).astype(np.float64)
    x = z @ rng.standard_normal((8, V)) + 0.3 * rng.standard_normal((n, V))
    x = (x - x.mean(0)) / x.std(0)
    return (sig(x) if bernoulli else x).astype(np.float32)


def params(stack, seed=7):
    """weights 0.1 N(0,1); hidden AND visible biases 0.1 N(0,1), so that a weight cost wrongly applied to a bias shows."""
    rng = np.random.default_rng(seed + sum(stack.sizes))
    L = len(stack.sizes)
    W, c, a = [None] * L, [None] * L, [None] * L
    for l in range(1, L):
        W[l] = (0.1 * rng.standard_normal((stack.sizes[l - 1], stack.sizes[l]))).astype(np.float32)
        c[l] = (0.1 * rng.standard_normal(stack.sizes[l])).astype(np.float32)
        a[l] = (0.1 * rng.standard_normal(stack.sizes[l - 1])).astype(np.float32)
    return W, c, a


def cd1(v0, W, c, a, visible, sample, u=None):
    """One CD-1 pass in float64: dict of p0 s0 v1 p1 gw gc ga pos recon."""
    f = lambda x: np.asarray(x, np.float64)
    v0, W, c, a = f(v0), f(W), f(c), f(a)
    p0 = sig(v0 @ W + c)
    s0 = (u < p0.astype(np.float32)).astype(np.float64) if sample else p0
    z = s0 @ W.T + a
    v1 = sig(z) if visible else z
    p1 = sig(v1 @ W + c)
    pos = v0.T @ p0
    return dict(v0=v0, p0=p0, s0=s0, v1=v1, p1=p1, pos=pos, gw=v1.T @ p1 - pos, gc=(p1 - p0).sum(0), ga=(v1 - v0).sum(0),
                recon=float(((v0 - v1) ** 2).sum()))


def update(hy, B, w, d, g, is_weight):
    """d' = m d - lrate (g / B + wc w), w' = w + d' in float64, with the hyper-parameters as fp32 holds them; (d', w')."""
    f32 = lambda v: float(np.float32(v))
    m, lr, wc = f32(hy.momentum), f32(hy.lrate), f32(hy.weightcost) if is_weight else 0.0
    w, d, g = (np.asarray(x, np.float64) for x in (w, d, g))
    dn = m * d - lr * (g / B + wc * w)
    return dn, w + dn


def relmax(got, ref, scale=None):
    ref = np.asarray(ref, np.float64)
    s = np.abs(ref).max() if scale is None else scale
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(s, 1e-300))


def stage_errors(tr, W, c, a, visible, sample, u):
    """Every stage of the trace `tr` (a dict of arrays as RBMStack.step returns it) against float64 on the trace's own operands:
    {stage: error in units of its bar}.  s0 is exact: 0 or inf."""
    f = lambda x: np.asarray(x, np.float64)
    v0, p0, s0, v1, p1 = (f(tr[k]) for k in ("v0", "p0", "s0", "v1", "p1"))
    W, c, a = f(W), f(c), f(a)
    e = {}
    e["p0"] = relmax(p0, sig(v0 @ W + c)) / GEMM_BAR
    s0_ref = (u < np.asarray(tr["p0"], np.float32)).astype(np.float32) if sample else np.asarray(tr["p0"], np.float32)
    e["s0"] = 0.0 if np.array_equal(np.asarray(tr["s0"], np.float32), s0_ref) else float("inf")
    z = s0 @ W.T + a
    e["v1"] = relmax(v1, sig(z) if visible else z) / GEMM_BAR
    e["p1"] = relmax(p1, sig(v1 @ W + c)) / GEMM_BAR
    pos = v0.T @ p0
    e["gw"] = relmax(tr["gw"], v1.T @ p1 - pos, np.abs(pos).max()) / GEMM_BAR
    e["gc"] = relmax(tr["gc"], (p1 - p0).sum(0), p0.sum(0).max()) / GEMM_BAR
    e["ga"] = relmax(tr["ga"], (v1 - v0).sum(0), np.abs(v0).sum(0).max()) / GEMM_BAR
    d32 = np.asarray(tr["v0"], np.float32) - np.asarray(tr["v1"], np.float32)
    ref = float((d32.astype(np.float64) ** 2).sum())
    e["recon"] = abs(tr["recon"] - ref) / max(ref, 1e-300) / RECON_BAR
    return e


def update_errors(hy, B, old, state, grads, new):
    """The applied step against float64 from the stored gradients: old / new = (W, c, a), state = (dW, dc, da) before the step,
    grads = (gw, gc, ga).  {tensor: error in units of UPDATE_BAR}, and the new state in float64."""
    e, nstate = {}, []
    for name, w, d, g, wn, isw in zip(("W", "c", "a"), old, state, grads, new, (True, False, False)):
        dn, ref = update(hy, B, w, d, g, isw)
        e[name] = relmax(wn, ref) / UPDATE_BAR
        nstate.append(dn)
    return e, tuple(nstate)


def meanfield_steps(X, B, W, c, a, visible, hy, n_steps):
    """n_steps applied CD-1 steps with sample = 0 on consecutive bunches of X, in float64: (W, c, a) and the recon of every step."""
    W, c, a = (np.asarray(x, np.float64).copy() for x in (W, c, a))
    dW, dc, da = np.zeros_like(W), np.zeros_like(c), np.zeros_like(a)
    rec = []
    for i in range(n_steps):
        r = cd1(X[i * B:(i + 1) * B], W, c, a, visible, False)
        rec.append(r["recon"])
        dW, W = update(hy, B, W, dW, r["gw"], True)
        dc, c = update(hy, B, c, dc, r["gc"], False)
        da, a = update(hy, B, a, da, r["ga"], False)
    return (W, c, a), rec


# ------------------------------------------------------------------ the mutants
MUTANTS = ("negative_phase_dropped", "gw_sign_flipped", "p0_for_s0_in_down_pass", "pad_columns_at_half", "rows_past_bunch_in_statistics",
           "lrate_times_one_minus_m", "weight_cost_on_a_bias", "g_not_divided_by_bunch", "bernoulli_visibles_left_linear")
CAUGHT_BY = {"negative_phase_dropped": "gw", "gw_sign_flipped": "gw", "p0_for_s0_in_down_pass": "v1", "pad_columns_at_half": "v1",
             "rows_past_bunch_in_statistics": "gw", "lrate_times_one_minus_m": "W", "weight_cost_on_a_bias": "c",
             "g_not_divided_by_bunch": "W", "bernoulli_visibles_left_linear": "v1"}


def _as_trace(r):
    t = {k: r[k].astype(np.float32) for k in ("v0", "p0", "s0", "v1", "p1", "gw", "gc", "ga")}
    d32 = t["v0"] - t["v1"]
    t["recon"] = float((d32.astype(np.float64) ** 2).sum())
    return t


def miss(name, stack_id="S", hset="A"):
    """By how many bars the check CAUGHT_BY[name] misses the mutant, float64 standing in for a faultless device.  Gaussian layer 1
    of the stack, except for the Bernoulli mutant (sigma of the rows as visibles).  The unmutated trace is inside every bar
    (test_rbm_host.py asserts that beside each mutant)."""
    st, hy = STACKS[stack_id], HYPER[hset]
    B, V, H = st.bunch, st.sizes[0], st.sizes[1]
    visible = 1 if name == "bernoulli_visibles_left_linear" else 0
    X = rows(st, bernoulli=bool(visible))
    W, c, a = (x[1] for x in params(st))
    u = uniforms(SEED, 0, 1, B, H)
    r = cd1(X[:B], W, c, a, visible, True, u)
    stage = CAUGHT_BY[name]
    if name == "negative_phase_dropped":
        r["gw"] = r["v1"].T @ r["p1"]
    elif name == "gw_sign_flipped":
        r["gw"] = -r["gw"]
    elif name == "p0_for_s0_in_down_pass":
        r["v1"] = r["p0"] @ np.asarray(W, np.float64).T + a
    elif name == "bernoulli_visibles_left_linear":
        r["v1"] = r["s0"] @ np.asarray(W, np.float64).T + a
    elif name == "rows_past_bunch_in_statistics":
        # the rows between B and the tile's end hold what the passes compute from zero input rows, and the statistics count them
        pad = pad64(B) - B
        assert pad > 0
        z = cd1(np.zeros((pad, V)), W, c, a, visible, False)
        r["gw"] = r["gw"] + z["v1"].T @ z["p1"] - z["v0"].T @ z["p0"]
    elif name == "pad_columns_at_half":
        # two applied steps in which the pad columns of p0 / s0 / p1 hold sigma(0) and the update runs over the padded W: the pad
        # columns of W leave zero, and the third step's down pass reads them against s0's pad columns
        Hp = pad64(H)
        assert Hp > H
        Wp, dWp = np.zeros((V, Hp)), np.zeros((V, Hp))
        Wp[:, :H] = W
        for i in range(2):
            q = cd1(X[i * B:(i + 1) * B], Wp[:, :H], c, a, visible, False)
            g = np.zeros((V, Hp))
            g[:, :H] = q["gw"]
            g[:, H:] = (0.5 * (q["v1"] - q["v0"]).sum(0))[:, None]
            dWp, Wp = update(hy, B, Wp, dWp, g, True)
        r = cd1(X[2 * B:3 * B], Wp[:, :H], c, a, visible, True, u)
        r["v1"] = r["v1"] + 0.5 * Wp[:, H:].sum(1)[None, :]
        W = Wp[:, :H]
    if stage in ("gw", "v1"):
        return stage_errors(_as_trace(r), W, c, a, visible, True, u)[stage]
    # the update mutants: one applied step from zero state
    f32 = lambda v: float(np.float32(v))
    m, lr, wc = f32(hy.momentum), f32(hy.lrate), f32(hy.weightcost)
    g = {"W": r["gw"], "c": r["gc"], "a": r["ga"]}[stage]
    w = np.asarray({"W": W, "c": c, "a": a}[stage], np.float64)
    wc_t = wc if stage == "W" else 0.0
    if name == "lrate_times_one_minus_m":
        lr = (1.0 - m) * lr
    elif name == "weight_cost_on_a_bias":
        wc_t = wc
    div = 1.0 if name == "g_not_divided_by_bunch" else float(B)
    got = w - lr * (g / div + wc_t * w)
    _, ref = update(hy, B, w, np.zeros_like(w), g, stage == "W")
    return relmax(got, ref) / UPDATE_BAR
