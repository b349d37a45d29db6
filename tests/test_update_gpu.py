"""The momentum update with weight cost, and the bf16 shadow of the weights, in every update kernel the step can dispatch (-m gpu).

Per case of the dispatch matrix and hyper set of tests/update_cases.py (rule 0, m 0.9, wc 1/16 | rule 1, m 0.75, wc 1/64; the
matrices themselves run wc 0, m 0.5, rule 0, where `wc * w` vanishes and `m` equals `1 - m`), on the device's OWN operands:

  step one    T.train on bunch 0 from zero momentum against update_cases.restate of (W0, 0, G0), G0 the gradient a twin handle
              made from (W0, b0) stores for the same bunch (grads_resident / read_grads);
  shadow one  a handle F1 made fresh from T's (W1, b1) must forward, cross-validate and differentiate bit for bit as T does: on a
              bf16 handle T reads the shadow its update epilogue wrote, F1 the one bp_to_bf16_both makes at creation, the forward reads
              it as it lies and the dgrad transposed -- a shadow element that is not f2bf of its master weight shows in one of the three;
  step two    T.train_resident on bunch 1 with the carried momentum against restate of (W1, D1, G1), G1 from F1;
  shadow two  the same against F2 made from (W2, b2): the shadow written from non-zero momentum.

fp32 handles run the same procedure; the shadow checks then pin that get_weights -> create is the identity.

Bar for the two steps: update_cases.BAR = 1e-5 of max|expected| per tensor (its docstring says why); tests/test_update_host.py shows
on the CPU that the restatement meets it and that five wrong updates miss it by more than 1000 x.  The shadow checks are
np.array_equal.  Every measured value and every count of unequal words goes to the parity record."""
import numpy as np
import pytest

import dispatch_cases as DC
import update_cases as UC
from test_dispatch_gpu import worst_block

pytestmark = pytest.mark.gpu


def _mk(pkg, c, h, W, b, cap):
    kw = dict(activation=c.act, compute_dtype=c.dtype, max_chunk_frames=cap, momentum_rule=h.rule)
    if c.out is not None:
        kw.update(output_activation=1, output_linear_cols=c.out[0], output_loss=c.out[1])
    return pkg.BP_GPU(1, len(c.ls), c.ls, c.B, h.lr, h.m, h.wc, W, b, **kw)


def _state(g):
    (w, b), (dw, db) = g.get_weights(), g.get_deltas()
    return dw, db, w, b


def _stored_gradient(g, x, t):
    """The gradient of the first bunch of (x, t) as the store kernels leave it: (unpadded, padded)."""
    g.upload_chunk(x, t)
    g.grads_resident(0)
    return g.read_grads(), g.read_grads(padded=True)


def _unequal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return int(a.size - np.count_nonzero((a == b) | (np.isnan(a) & np.isnan(b))))


def _check_step(c, what, got, want, errs_out, fails):
    errs, triples = UC.errors(got, want)
    errs_out[what] = errs
    for name, a, r in triples:
        if not errs[name] < UC.BAR:
            fails.append("%s %s: %.3e (bar %.0e); %s" % (what, name, errs[name], UC.BAR, worst_block(a, r)))


def _check_shadow(c, what, T, F, x, t, counts, fails, grads=None):
    """T and F hold the same master weights: the same forward, the same CV sum (and the same stored gradient) to the last bit."""
    B, n = c.B, 2 * c.B + c.B // 2
    a, b = T.forward(x[:B + 3]), F.forward(x[:B + 3])
    counts[what + " forward"] = _unequal(a, b)
    if counts[what + " forward"]:
        fails.append("%s: forward of the trained handle differs from a handle made from its weights in %d of %d words; %s" % (
            what, counts[what + " forward"], a.size, worst_block(a, b)))
    cv = T.CrossValid(n, x, t), F.CrossValid(n, x, t)
    counts[what + " cv_sum"] = int(cv[0] != cv[1])
    if cv[0] != cv[1]:
        fails.append("%s: CV sums %r and %r" % (what, cv[0], cv[1]))
    if grads is not None:
        (pw, pb), (qw, qb) = grads
        for l in range(1, len(c.ls)):
            for name, p, q in (("G%d" % l, pw[l], qw[l]), ("gb%d" % l, pb[l], qb[l])):
                counts["%s %s" % (what, name)] = _unequal(p, q)
                if counts["%s %s" % (what, name)]:
                    fails.append("%s: padded gradient buffer %s differs in %d of %d words; %s" % (what, name, counts["%s %s" % (what, name)], p.size, worst_block(p, q)))


@pytest.mark.parametrize("c,hset", UC.RUNS, ids=UC.RUN_IDS)
def test_update_and_shadow(pkg, parity_record, c, hset):
    h, B = UC.hyper(hset, c.dtype), c.B
    n = 2 * B + B // 2
    W0, b0, x, t = DC.case_data(c, n)
    x0, t0, x1, t1 = x[:B], t[:B], x[B:2 * B], t[B:2 * B]
    errs, counts, fails = {}, {}, []

    twin = _mk(pkg, c, h, W0, b0, n)
    (gw0, gb0), _ = _stored_gradient(twin, x0, t0)
    twin.close()
    T = _mk(pkg, c, h, W0, b0, n)
    T.train(B, x0, t0)
    D1, d1, W1, b1 = s1 = _state(T)
    Z, z = UC.zeros_like_state(W0, b0)
    _check_step(c, "step one", s1, UC.restate(h, B, W0, b0, Z, z, gw0, gb0), errs, fails)

    F1 = _mk(pkg, c, h, W1, b1, n)
    (gw1, gb1), padded_f = _stored_gradient(F1, x1, t1)
    _, padded_t = _stored_gradient(T, x1, t1)
    after = _state(T)                                              # (grads_resident leaves the state alone)
    assert all(np.array_equal(p[l], q[l]) for p, q in zip(s1, after) for l in range(1, len(c.ls))), (c.id, "grads_resident changed the state")
    _check_shadow(c, "shadow one", T, F1, x, t, counts, fails, grads=(padded_t, padded_f))
    F1.close()

    T.upload_chunk(x1, t1)                                          # (CrossValid brought its own chunk)
    T.train_resident(0, B)
    T.sync()
    s2 = _state(T)
    _check_step(c, "step two", s2, UC.restate(h, B, W1, b1, D1, d1, gw1, gb1), errs, fails)

    F2 = _mk(pkg, c, h, s2[2], s2[3], n)
    _check_shadow(c, "shadow two", T, F2, x, t, counts, fails)
    F2.close()
    T.close()

    moved = min(float(np.abs(np.asarray(s2[0][l], np.float64) - 0.0).max()) for l in range(1, len(c.ls)))
    print(c.id, hset, "update errors", errs, "unequal words", counts)
    parity_record(update={"hyper": h._asdict(), "errors": errs, "bar": UC.BAR, "worst": max(max(e.values()) for e in errs.values())},
                  shadow={"unequal": counts})
    assert moved > 0.0, (c.id, "a layer's momentum state is all zero after two steps")
    assert not fails, (c.id, hset, fails)
