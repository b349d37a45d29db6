"""The device against the oracle, bit for bit (-m gpu), on data whose arithmetic is exact: tests/exact_data.py has the recipe and the
three conditions under which every GEMM of the step gives the same fp32 numbers in any summation order, tests/test_exact_host.py
checks them on the CPU.  The cases, nets and bunches are those of tests/dispatch_cases.py, with ReLU in the hidden layers.

Where tests/test_dispatch_gpu.py can only ask 2e-2 rms of a bf16 gradient (two correct bf16 implementations differ by that much),
these tests ask np.array_equal: an indexing, k-tail, tile-map, k-split, ring or padding defect is an exact mismatch in a nameable
64 x 64 block.  Held exactly: the gradient through the store kernels (first and second bunch of a chunk), one fused step from zero
momentum, the forward on the linear columns and the CV sum -- every bf16 case, with dropout on three of them, and the gradient of a shard handle
at an unaligned rank offset on two; of the fp32 cases the
forward and CV sum of all, the gradient and step of those whose bunch is a power of two (2/B must be an fp32 number).  A failure
names the tensor, the worst block, the number of unequal elements, their size in ulps and the first unequal pair as hex words; the
counts go to the parity record (all zeros when green)."""
import numpy as np
import pytest

import dispatch_cases as DC
import exact_data as X

pytestmark = pytest.mark.gpu

STEP_RUNS = [(cid, drop) for cid, drop in X.exact_runs() if X.steps_exactly(DC.BY_ID[cid])]
_ids = lambda runs: ["%s%s" % (cid, "-dropout" if drop else "") for cid, drop in runs]


def _mk(pkg, p, cap, drop, **extra):
    c = p.c
    kw = dict(activation=0, compute_dtype=c.dtype, max_chunk_frames=cap, **extra)
    if c.out is not None:
        kw.update(output_activation=1, output_linear_cols=c.out[0], output_loss=c.out[1])
    if drop:
        kw.update(X.DROP)
    return pkg.BP_GPU(1, len(c.ls), c.ls, c.B, X.LR, X.MOM, X.WC, p.W, p.b, **kw)


def _gradient_against(g, p, ref, what, counts):
    """The flat gradient buffer of the last grads_resident against the oracle's (gw, gb): equal on the true extent, 0.0 on every
    pad row and pad column.  Returns the failure texts."""
    c, fails = p.c, []
    pw, pb = g.read_grads(padded=True)
    for l in range(1, len(c.ls)):
        prev, cur = c.ls[l - 1], c.ls[l]
        for name, a, r in (("G%d" % l, pw[l][:prev, :cur], ref[0][l]), ("gb%d" % l, pb[l][:cur], ref[1][l])):
            counts["%s %s" % (what, name)] = X.count_unequal(a, r)
            msg = X.unequal("%s %s" % (what, name), a, r)
            if msg:
                fails.append(msg)
        pads = int(np.count_nonzero(pw[l][prev:, :])) + int(np.count_nonzero(pw[l][:, cur:])) + int(np.count_nonzero(pb[l][cur:]))
        counts["%s pad of layer %d" % (what, l)] = pads
        if pads:
            fails.append("%s: %d pad words of layer %d are not 0.0, first rows %s, first columns %s" % (
                what, pads, l, np.argwhere(pw[l][prev:, :] != 0)[:3].tolist(), np.argwhere(pw[l][:, cur:] != 0)[:3].tolist()))
    return fails


@pytest.mark.parametrize("cid,drop", STEP_RUNS, ids=_ids(STEP_RUNS))
def test_gradient_store_is_exact(pkg, oracle_mod, parity_record, cid, drop):
    """grads_resident(0) on a chunk of B + B/2 frames, then grads_resident(B) on one of 2B + B/2 (the second bunch: the chunk-offset
    addressing; its targets come from that bunch's reference outputs)."""
    p, r = X.problem(cid, drop), X.reference(cid, drop)
    B = p.c.B
    g = _mk(pkg, p, 2 * B + B // 2, drop)
    counts = {}
    g.upload_chunk(p.x[:B + B // 2], p.t[:B + B // 2])
    g.grads_resident(0)
    fails = _gradient_against(g, p, r.grads[0], "first bunch", counts)
    g.upload_chunk(p.x, p.t)
    g.grads_resident(B)
    fails += _gradient_against(g, p, r.grads[1], "second bunch", counts)
    g.close()
    print(cid, "gradient, unequal elements:", counts)
    parity_record(exact_gradient={"unequal": counts})
    assert not fails, (cid, fails)


@pytest.mark.parametrize("cid", X.SHARD_CASES)
def test_shard_gradient_store_is_exact(pkg, oracle_mod, parity_record, cid):
    """The same on a shard handle with dropout: bunch B of a global bunch 2B at rank_frame_offset 3, so the gradient is scaled by
    2/(2B) and the masks are those of the global frames 3 .. B + 2, drawn through the last two-block branch of drop_words4 in the
    64-row and both 128-row hidden forwards.  A shard handle trains only through its group: gradient store alone."""
    shard = X.shard_of(cid)
    p, r = X.problem(cid, True, shard), X.reference(cid, True, shard=shard)
    B = p.c.B
    g = _mk(pkg, p, 2 * B + B // 2, True, global_bunchsize=shard[1], rank_frame_offset=shard[0])
    counts = {}
    g.upload_chunk(p.x, p.t)
    g.grads_resident(0)
    fails = _gradient_against(g, p, r.grads[0], "first bunch", counts)
    g.grads_resident(B)
    fails += _gradient_against(g, p, r.grads[1], "second bunch", counts)
    g.close()
    print(cid, "shard gradient at offset %d of a global bunch %d, unequal elements:" % shard, counts)
    parity_record(exact_gradient={"unequal": counts})
    assert not fails, (cid, fails)


@pytest.mark.parametrize("cid,drop", STEP_RUNS, ids=_ids(STEP_RUNS))
def test_fused_step_is_exact(pkg, oracle_mod, parity_record, cid, drop):
    """train() on one bunch from zero momentum, lr 0.5, momentum 0.5, no weight cost: dW = -1/4 fl(G / B) in both implementations,
    one correctly rounded division and an exact scaling.  A tensor that differs from the oracle's by at most one fp32 ulp on every
    element, while the gradient buffer of the same handle configuration is exact, is an expression-rounding difference between
    the host and the device compiler: the one-ulp form is asserted for it and the parity record names it.  Anything larger fails."""
    p, r = X.problem(cid, drop), X.reference(cid, drop)
    c, B = p.c, p.c.B
    g = _mk(pkg, p, B, drop)
    g.train(B, p.x[:B], p.t[:B])
    got = g.get_weights() + g.get_deltas()
    g.close()
    counts, msgs, one_ulp = {}, {}, []
    for i, nm in enumerate(("W", "b", "dW", "db")):
        for l in range(1, len(c.ls)):
            name = "%s%d" % (nm, l)
            counts[name] = X.count_unequal(got[i][l], r.state[i][l])
            if counts[name]:
                msgs[name] = X.unequal(name, got[i][l], r.state[i][l])
                if X.within_one_ulp(got[i][l], r.state[i][l]):
                    one_ulp.append(name)
    fails = [m for name, m in msgs.items() if name not in one_ulp]
    if one_ulp and not fails:                                      # the fallback is owed only to an exact gradient buffer
        g = _mk(pkg, p, B, drop)
        g.upload_chunk(p.x[:B], p.t[:B])
        g.grads_resident(0)
        fails = _gradient_against(g, p, r.grads[0], "gradient buffer", {})
        g.close()
        if fails:
            fails += [msgs[name] for name in one_ulp]
    print(cid, "fused step, unequal elements:", counts, "one-ulp form needed for", one_ulp)
    parity_record(exact_fused_step={"unequal": counts, "one_ulp_form": one_ulp})
    assert not fails, (cid, fails)
    for name in one_ulp:
        print(cid, name, "holds in the one-ulp form only:", msgs[name])


@pytest.mark.parametrize("cid", [c.id for c in DC.CASES])
def test_forward_and_cv_are_exact(pkg, oracle_mod, parity_record, cid):
    """forward() on B + 3 frames: equal on the linear columns (the logistic ones stay with tests/test_dispatch_gpu.py).  CrossValid
    on 2B + B/2 frames against targets that are 0, 1 or 2 away from the reference output: the sum of squares is an integer below
    2^24 and any order of summation gives it.  A logistic case has no exact sum: the CV comparison is skipped with the reason."""
    p, r = X.problem(cid), X.reference(cid)
    c, B = p.c, p.c.B
    lin = c.ls[-1] if c.out is None else c.out[0]
    g = _mk(pkg, p, 2 * B + B // 2, False)
    out = g.forward(p.x[:B + 3])
    cv = g.CrossValid(p.x.shape[0], p.x, p.t_cv)
    g.close()
    counts = {"forward": X.count_unequal(out[:, :lin], r.forward[:, :lin])}
    fails = [m for m in [X.unequal("forward (linear columns)", out[:, :lin], r.forward[:, :lin])] if m]
    if p.cv_sum is None:
        print(cid, "CV comparison skipped:", p.cv_skip)
    else:
        counts["cv_sum"] = int(cv != r.cv)
        if cv != r.cv:
            fails.append("CV sum: got %r (%s), the oracle's %r (%s)" % (cv, float(cv).hex(), r.cv, float(r.cv).hex()))
    print(cid, "forward / CV, unequal elements:", counts)
    parity_record(exact_forward_and_cv={"unequal": counts, "cv_skipped": p.cv_skip})
    assert not fails, (cid, fails)
