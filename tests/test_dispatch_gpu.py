"""The dispatch matrix (-m gpu): every GEMM-family kernel the step can launch, run once at a shape that reaches it and held
against a reference of the same operation.  The table is tests/dispatch_cases.py; tests/dispatch_np.py says which kernels a
case reaches and tests/test_dispatch_coverage.py (no GPU) that together they reach all of them.

Reference: oracle.Oracle (fp32, or compute_dtype=1 for bf16 cases).  The oracle has no logistic output layer; those cases use the
float64 references of tests/output_ref.py (torch autograd for fp32, the hand-written bf16-storage form for bf16).

Bars -- none of them new:
  fp32   util.TOL (1e-4, max|a - ref| / max|ref| per tensor) on everything; the one-bunch gradient and the layer outputs
         additionally 1e-5 (the bar of test_gradient_buffer_matches_oracle_and_fused_step) where the oracle's own spread between fp32
         and fp64 accumulation supports it (dispatch_cases.strict_bar).
  bf16   the formulas of test_bf16_step_matches_bf16_oracle: forward 2e-3 against the bf16 reference, W and b at TOL_BF16 / 4,
         gradients and momentum state 2e-2 rms; cases deeper or wider than that test's add 1.5 x the oracle's spread, the rule of
         test_bf16_config5_shape_one_step.
  The ignored-frames and padding checks are exact.

Two passes turn on switches of the forward epilogues that the 24 cases leave at rest (tests/switch_cases.py has the table): the
gradient, the fused step and the trajectory once more over dispatch_cases.LOSS1_CASES (output_loss 1 on every logistic output
kernel), forward and CV once more on a dropout handle (alpha = 1 - omit in every forward kernel).  Same bars."""
import numpy as np
import pytest

import dispatch_cases as DC
from util import TOL, relerr

pytestmark = pytest.mark.gpu

TOL_BF16 = 2e-2
LR = {0: 1.0, 1: 0.5}            # fp32 / bf16 cases (the rates of test_train_matches_oracle / test_bf16_step_matches_bf16_oracle)
MOM = 0.5


def relerr_rms(a, ref):
    a = np.asarray(a, np.float64); ref = np.asarray(ref, np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum()) / max(np.sqrt((ref ** 2).sum()), 1e-30))


def worst_block(a, ref):
    """The 64 x 64 block with the largest error, as text: a wrong tile can be read from a failure message."""
    a = np.atleast_2d(np.asarray(a, np.float64)); ref = np.atleast_2d(np.asarray(ref, np.float64))
    d = np.abs(a - ref)
    r, c = np.unravel_index(int(d.argmax()), d.shape)
    r0, c0 = (r // 64) * 64, (c // 64) * 64
    blk = d[r0:r0 + 64, c0:c0 + 64]
    return "worst 64x64 block rows %d.., cols %d.. (of %s): max|err| %.3e at [%d, %d], %d of %d elements above 1e-3 of max|ref|" % (
        r0, c0, d.shape, d.max(), r, c, int((blk > 1e-3 * max(np.abs(ref).max(), 1e-30)).sum()), blk.size)


def _mk(pkg, c, W, b, cap, **extra):
    kw = dict(activation=c.act, compute_dtype=c.dtype, max_chunk_frames=cap, **extra)
    if c.out is not None:
        kw.update(output_activation=1, output_linear_cols=c.out[0], output_loss=c.out[1])
    return pkg.BP_GPU(1, len(c.ls), c.ls, c.B, LR[c.dtype], MOM, 0.0, W, b, **kw)


# ------------------------------------------------------------------ references with one interface
class OracleRef(object):
    def __init__(self, oracle_mod, c, W, b, acc_double=False, drop=None):
        self.o = oracle_mod.Oracle(c.ls, c.B, LR[c.dtype], MOM, 0.0, W, b, activation=c.act, compute_dtype=c.dtype, acc_double=acc_double,
                                   **(drop or {}))

    def grads(self, x, t):
        gw, gb, ys, _ = self.o.grads(x, t)
        return gw, gb, ys

    def forward(self, x):
        return self.o.forward(x)

    def cv(self, x, t):
        return self.o.crossvalid(x, t)

    def train(self, x, t):
        self.o.train(x, t)
        return self.o.W, self.o.b, self.o.dW, self.o.db


class LogisticRef(object):
    """float64 state; fp32 cases: torch autograd (output_ref.ref_grads, asked of a child process: output_ref.in_child says why),
    bf16 cases: bf16 storage written out by hand."""

    def __init__(self, c, W, b, drop=None):
        L = len(c.ls)
        self.c, self.L = c, L
        self.keep = DC.keep_scales(c, drop) if drop else None          # forward and CV of a dropout handle
        self.W = [None] + [np.asarray(W[l], np.float64).copy() for l in range(1, L)]
        self.b = [None] + [np.asarray(b[l], np.float64).copy() for l in range(1, L)]
        self.dW = [None] + [np.zeros_like(self.W[l]) for l in range(1, L)]
        self.db = [None] + [np.zeros_like(self.b[l]) for l in range(1, L)]

    def grads(self, x, t):
        import output_ref as R
        c = self.c
        if c.dtype == 1:
            gw, gb, ys, _ = R.bf16_logistic_grads(c.ls, self.W, self.b, x, t, c.act, c.out[0], c.out[1])
            return gw, gb, ys
        return R.in_child("grads", c.ls, self.W, self.b, x, t, act=c.act, lin=c.out[0], loss=c.out[1])

    def forward(self, x):
        import output_ref as R
        c = self.c
        if c.dtype == 1:
            return R.bf16_logistic_grads(c.ls, self.W, self.b, x, None, c.act, c.out[0], c.out[1], keep=self.keep)[3]
        return R.in_child("forward", c.ls, self.W, self.b, x, act=c.act, lin=c.out[0], keep=self.keep)

    def cv(self, x, t):
        return float(((self.forward(x) - t.astype(np.float64)) ** 2).sum())

    def train(self, x, t):
        import output_ref as R
        c, B, c1 = self.c, self.c.B, (1.0 - MOM) * LR[self.c.dtype]
        if c.dtype == 0:
            self.W, self.b, self.dW, self.db = R.in_child("train", c.ls, self.W, self.b, x, t, act=c.act, lin=c.out[0], loss=c.out[1], B=B,
                                                          steps=x.shape[0] // B, lr=LR[0], m=MOM)
            return self.W, self.b, self.dW, self.db
        for i in range(x.shape[0] // B):                          # (the trailing partial bunch is ignored)
            gw, gb, _ = self.grads(x[i * B:(i + 1) * B], t[i * B:(i + 1) * B])
            for l in range(1, self.L):
                self.dW[l] = MOM * self.dW[l] - c1 * (gw[l] / B); self.W[l] = self.W[l] + self.dW[l]
                self.db[l] = MOM * self.db[l] - c1 * (gb[l] / B); self.b[l] = self.b[l] + self.db[l]
        return self.W, self.b, self.dW, self.db


def _ref(oracle_mod, c, W, b, drop=None):
    return OracleRef(oracle_mod, c, W, b, drop=drop) if c.out is None else LogisticRef(c, W, b, drop=drop)


def _spread_after_training(oracle_mod, c, W, b, x, t):
    """bf16, deep or wide cases: rms spread of the oracle's momentum state between fp32 and fp64 accumulation, per tensor."""
    if not (c.dtype == 1 and DC.deep_or_wide(c) and c.out is None):
        return None
    a, d = OracleRef(oracle_mod, c, W, b), OracleRef(oracle_mod, c, W, b, acc_double=True)
    (_, _, aw, ab), (_, _, dw, db) = a.train(x, t), d.train(x, t)
    return {"dW%d" % l: relerr_rms(aw[l], dw[l]) for l in range(1, len(c.ls))}, {"db%d" % l: relerr_rms(ab[l], db[l]) for l in range(1, len(c.ls))}


def _check_state(c, got, ref, spread, what, parity_record):
    """W, b, dW, db after training against the reference's, at the bars of the module docstring."""
    (w, bb, dw, dbb), (rw, rb, rdw, rdb) = got, ref
    errs, bars, fails = {}, {}, []
    for l in range(1, len(c.ls)):
        for name, a, r, kind in (("W%d" % l, w[l], rw[l], "p"), ("b%d" % l, bb[l], rb[l], "p"), ("dW%d" % l, dw[l], rdw[l], "d"), ("db%d" % l, dbb[l], rdb[l], "d")):
            if c.dtype == 0:
                e, bar = relerr(a, r), TOL
            elif kind == "p":
                e, bar = relerr(a, r), TOL_BF16 / 4
            else:
                e, bar = relerr_rms(a, r), TOL_BF16 + (1.5 * {**spread[0], **spread[1]}[name] if spread else 0.0)
            errs[name], bars[name] = e, bar
            if not e < bar:
                fails.append("%s: %.3e (bar %.3e); %s" % (name, e, bar, worst_block(a, r)))
    print(c.id, what, errs)
    parity_record(**{what: {"errors": errs, "bars": bars}})
    assert not fails, (c.id, what, fails)


@pytest.fixture(params=DC.CASES, ids=[c.id for c in DC.CASES])
def case(request):
    return request.param


@pytest.fixture(params=DC.LOSS1_CASES, ids=[c.id for c in DC.LOSS1_CASES])
def loss1_case(request):
    """The logistic cases at output_loss 1 (tests/switch_cases.py: the switch `loss`)."""
    return request.param


# ------------------------------------------------------------------ 1. one bunch's gradient through the store kernels
def test_gradient_store(pkg, oracle_mod, parity_record, case):
    _gradient_store(pkg, oracle_mod, parity_record, case)


def test_gradient_store_loss1(pkg, oracle_mod, parity_record, loss1_case):
    """The same at output_loss 1: d *= o (1 - o) on the logistic columns of every logistic output kernel; same bars."""
    _gradient_store(pkg, oracle_mod, parity_record, loss1_case)


def _gradient_store(pkg, oracle_mod, parity_record, case):
    """grads_resident + read_grads against the reference's gradient (fp32 handles: every hidden layer's output too), and every pad
    row and pad column of the flat gradient buffer exactly 0.0."""
    c, L = case, len(case.ls)
    n = c.B + c.B // 2
    W, b, x, t = DC.case_data(c, n)
    g = _mk(pkg, c, W, b, cap=n)
    g.upload_chunk(x, t)
    g.grads_resident(0)
    gw, gb = g.read_grads()
    pw, pb = g.read_grads(padded=True)
    ys_g = [g.read_layer_output(l) for l in range(1, L - 1)] if c.dtype == 0 else []
    g.close()
    rw, rb, ys = _ref(oracle_mod, c, W, b).grads(x[:c.B], t[:c.B])
    spread_now = DC.oracle_spread(c)
    if c.dtype == 0:
        bar = 1e-5 if DC.strict_bar(spread_now) else TOL
        assert DC.strict_bar(spread_now) == DC.strict_bar(c.spread), (c.id, "the table's spread", c.spread, "measured now", spread_now)
    else:
        bar = TOL_BF16 + (1.5 * spread_now if DC.deep_or_wide(c) and spread_now is not None else 0.0)
    err = relerr if c.dtype == 0 else relerr_rms
    errs, fails = {}, []
    for l in range(1, L):
        for name, a, r in (("G%d" % l, gw[l], rw[l]), ("gb%d" % l, gb[l], rb[l])):
            errs[name] = err(a, r)
            if not errs[name] < bar:
                fails.append("%s: %.3e; %s" % (name, errs[name], worst_block(a, r)))
    for l, y in enumerate(ys_g, 1):
        errs["y%d" % l] = relerr(y, ys[l])
        if not errs["y%d" % l] < bar:
            fails.append("y%d: %.3e; %s" % (l, errs["y%d" % l], worst_block(y, ys[l])))
    print(c.id, "gradient", errs, "bar", bar, "oracle spread", spread_now)
    parity_record(gradient={"errors": errs, "bar": bar, "oracle_spread_fp32_vs_fp64_accumulation": spread_now, "table_spread": c.spread})
    assert not fails, (c.id, fails)
    for l in range(1, L):                                            # padding stays zero
        assert not pw[l][c.ls[l - 1]:, :].any(), (c.id, "pad rows of G%d" % l, np.argwhere(pw[l][c.ls[l - 1]:, :] != 0)[:4])
        assert not pw[l][:, c.ls[l]:].any(), (c.id, "pad columns of G%d" % l, np.argwhere(pw[l][:, c.ls[l]:] != 0)[:4])
        assert not pb[l][c.ls[l]:].any(), (c.id, "pad of gb%d" % l)
        assert np.array_equal(pw[l][:c.ls[l - 1], :c.ls[l]], gw[l])


# ------------------------------------------------------------------ 2. one fused step from zero momentum
def test_fused_step(pkg, oracle_mod, parity_record, case):
    _fused_step(pkg, oracle_mod, parity_record, case)


def test_fused_step_loss1(pkg, oracle_mod, parity_record, loss1_case):
    _fused_step(pkg, oracle_mod, parity_record, loss1_case)


def _fused_step(pkg, oracle_mod, parity_record, case):
    c = case
    W, b, x, t = DC.case_data(c, c.B)
    g = _mk(pkg, c, W, b, cap=c.B)
    g.train(c.B, x, t)
    got = g.get_weights() + g.get_deltas()
    g.close()
    ref = _ref(oracle_mod, c, W, b).train(x, t)
    _check_state(c, got, ref, _spread_after_training(oracle_mod, c, W, b, x, t), "fused_step", parity_record)


# ------------------------------------------------------------------ 3. forward and CV
def test_forward_and_cv(pkg, oracle_mod, parity_record, case):
    """Forward on B + 3 frames and CV on a chunk with a partial last bunch (the fp32 forward then launches with fewer rows than
    the padded bunch)."""
    _forward_and_cv(pkg, oracle_mod, parity_record, case, None)


def test_forward_and_cv_keep_scaled(pkg, oracle_mod, parity_record, case):
    """The same on a handle with dropout configured that never trains: every forward epilogue runs with alpha = 1 - omit (0.9 on
    the first weight layer, 0.8 on the others).  Reference: the oracle with the same keywords, which scales as
    test_train_matches_oracle relies on; logistic cases: the keep argument of tests/output_ref.py.  Same bars."""
    _forward_and_cv(pkg, oracle_mod, parity_record, case, DC.KEEP_DROP)


def _forward_and_cv(pkg, oracle_mod, parity_record, case, drop):
    c = case
    n = 2 * c.B + c.B // 2
    W, b, x, t = DC.case_data(c, n)
    g = _mk(pkg, c, W, b, cap=n, **(dict(drop, seed=41) if drop else {}))
    out = g.forward(x[:c.B + 3])
    cv = g.CrossValid(n, x, t)
    g.close()
    r = _ref(oracle_mod, c, W, b, drop)
    ro, rcv = r.forward(x[:c.B + 3]), r.cv(x, t)
    errs = {"forward": relerr(out, ro), "cv_sum": abs(cv - rcv) / abs(rcv)}
    bars = {"forward": TOL, "cv_sum": TOL} if c.dtype == 0 else {"forward": 2e-3, "cv_sum": TOL_BF16}
    print(c.id, "forward / CV", "keep-scaled" if drop else "", errs)
    parity_record(forward_and_cv={"errors": errs, "bars": bars, "keep_scaled": bool(drop)})
    assert errs["forward"] < bars["forward"], (c.id, errs, worst_block(out, ro))
    assert errs["cv_sum"] < bars["cv_sum"], (c.id, errs)


# ------------------------------------------------------------------ 4. a short trajectory
def test_short_trajectory(pkg, oracle_mod, parity_record, case):
    """Three bunches plus an ignored partial one."""
    _short_trajectory(pkg, oracle_mod, parity_record, case)


def test_short_trajectory_loss1(pkg, oracle_mod, parity_record, loss1_case):
    _short_trajectory(pkg, oracle_mod, parity_record, loss1_case)


def _short_trajectory(pkg, oracle_mod, parity_record, case):
    c = case
    n = 3 * c.B + c.B // 2
    W, b, x, t = DC.case_data(c, n)
    g = _mk(pkg, c, W, b, cap=n)
    g.train(n, x, t)
    got = g.get_weights() + g.get_deltas()
    g.close()
    ref = _ref(oracle_mod, c, W, b).train(x, t)
    _check_state(c, got, ref, _spread_after_training(oracle_mod, c, W, b, x, t), "trajectory", parity_record)


# ------------------------------------------------------------------ 5. ignored frames are ignored
def _ignored_run(pkg, ls, B, dtype, fill):
    """Two long chunks of `fill` (both chunk buffers), then three bunches plus a partial one whose rows are `fill`: the gradient
    of the last whole bunch (store kernels), then the training of the chunk (fused kernels)."""
    from oracle import bp_numpy as N
    W, b = N.glorot_net(ls, seed=5, beta=1.0)
    rng = np.random.default_rng(31)
    n, cap = 3 * B + B // 2, 8 * B
    x = rng.normal(size=(n, ls[0])).astype(np.float32); t = rng.normal(size=(n, ls[-1])).astype(np.float32)
    x[3 * B:] = fill; t[3 * B:] = fill
    g = pkg.BP_GPU(1, len(ls), ls, B, 1.0, 0.5, 0.0, W, b, compute_dtype=dtype, max_chunk_frames=cap)
    for _ in range(2):
        g.upload_chunk(np.full((cap, ls[0]), fill, np.float32), np.full((cap, ls[-1]), fill, np.float32))
    g.upload_chunk(x, t)
    g.grads_resident(2 * B)
    grads = g.read_grads(padded=True)
    g.train_resident(0, n)
    g.sync()
    state = g.get_weights() + g.get_deltas()
    g.close()
    return grads, state


@pytest.mark.parametrize("B", [12, 80, 100])
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_ignored_frames_are_ignored(pkg, dtype, B):
    """The trailing partial bunch and whatever lies behind the chunk in the chunk buffers must not reach the result: with NaN in
    those places training and the stored gradient equal, bit for bit, what zeros there give.  (The fp32 weight gradients run their
    k-loop over the frames in whole tiles of 32 or 16; the rows of the layer-1 operand past the bunch come from the chunk buffer.)"""
    ls = [70, 65, 130, 33]
    (gw_n, gb_n), st_n = _ignored_run(pkg, ls, B, dtype, np.nan)
    (gw_z, gb_z), st_z = _ignored_run(pkg, ls, B, dtype, 0.0)
    for l in range(1, len(ls)):
        assert np.isfinite(gw_n[l]).all() and np.isfinite(gb_n[l]).all(), ("store", l, int((~np.isfinite(gw_n[l])).sum()), "non-finite gradient words")
        assert np.array_equal(gw_n[l], gw_z[l]) and np.array_equal(gb_n[l], gb_z[l]), ("store", l)
        for k, name in enumerate(("W", "b", "dW", "db")):
            assert np.isfinite(st_n[k][l]).all(), ("fused", name, l, int((~np.isfinite(st_n[k][l])).sum()), "non-finite words")
            assert np.array_equal(st_n[k][l], st_z[k][l]), ("fused", name, l)
        assert gw_z[l].any() and not np.array_equal(st_z[0][l], 0 * st_z[0][l])


# ------------------------------------------------------------------ 6. padding stays zero
@pytest.mark.parametrize("B", [12, 80, 100])
@pytest.mark.parametrize("dtype", [0, 1], ids=["fp32", "bf16"])
def test_gradient_buffer_padding_stays_zero(pkg, dtype, B):
    """Odd widths: every pad row and pad column of every layer in the flat gradient buffer is exactly 0.0 after grads_resident,
    also when a fused step ran on the handle before."""
    from oracle import bp_numpy as N
    ls = [70, 65, 130, 33]
    W, b = N.glorot_net(ls, seed=5, beta=1.0)
    rng = np.random.default_rng(37)
    x = rng.normal(size=(2 * B, ls[0])).astype(np.float32); t = rng.normal(size=(2 * B, ls[-1])).astype(np.float32)
    g = pkg.BP_GPU(1, len(ls), ls, B, 1.0, 0.5, 0.0, W, b, compute_dtype=dtype, max_chunk_frames=2 * B)
    g.train(2 * B, x, t)
    g.grads_resident(B)
    pw, pb = g.read_grads(padded=True)
    g.close()
    for l in range(1, len(ls)):
        assert pw[l].shape == ((ls[l - 1] + 63) // 64 * 64, (ls[l] + 63) // 64 * 64)
        assert pw[l][:ls[l - 1], :ls[l]].any()
        assert not pw[l][ls[l - 1]:, :].any() and not pw[l][:, ls[l]:].any() and not pb[l][ls[l]:].any(), l
