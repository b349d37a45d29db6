"""The conditions under which tests/test_exact_gpu.py may ask for bit-equality, checked on the CPU from the reference alone
(tests/exact_data.py states them): (a) every GEMM of the step accumulates exactly in fp32 in any order, (b) the oracle's fp32 and
fp64 accumulation agree to the last bit, (c) the data can see a defect -- for every case and variant the GPU file runs.  No GPU."""
import numpy as np
import pytest

import dispatch_cases as DC
import dispatch_np as D
import exact_data as X

RUNS = X.exact_runs()


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    from oracle import oracle as O
    O.build()


@pytest.mark.parametrize("cid,drop", RUNS, ids=["%s%s" % (cid, "-dropout" if drop else "") for cid, drop in RUNS])
def test_conditions_hold(cid, drop):
    """(a), (b), (c) on both bunches of the chunk, with the Philox masks where the GPU file runs the case with dropout."""
    fails, fig = X.conditions(cid, drop)
    print(cid, "dropout" if drop else "", fig)
    assert not fails, (cid, fails)
    assert fig["max_over_q_log2"] < 24 and fig["q_min_log2"] >= -40


@pytest.mark.parametrize("cid", X.SHARD_CASES)
def test_shard_conditions_hold(cid):
    """The same for the shard problems (scale 2/Bg, masks from rank_frame_offset 3 on), and the data sees the offset: with the
    masks of offset 0 or 4 the reference gradient is another one in most places of every tensor."""
    shard = X.shard_of(cid)
    assert shard[0] & 3 == 3 and shard[1] == 2 * DC.BY_ID[cid].B
    fails, fig = X.conditions(cid, True, shard)
    print(cid, "shard", shard, fig)
    assert not fails, (cid, fails)
    p, r = X.problem(cid, True, shard), X.reference(cid, True, shard=shard)
    B = p.c.B
    for off in (0, 4):
        gw, gb = X.oracle(p.c, p.W, p.b, drop=True).grads(p.x[:B], p.t_oracle[:B], masks=X.masks(p.c, p.W, p.b, off), scale_frames=shard[1])[:2]
        for l in range(1, len(p.c.ls)):
            share = X.count_unequal(gw[l], r.grads[0][0][l]) / float(gw[l].size)
            assert share > 0.5, (cid, off, l, share)


def test_every_case_is_run_and_reaches_its_kernels():
    """Every bf16 case of the table runs gradient, step, forward and CV; ReLU in place of Sigmoid changes no kernel."""
    ran = set(cid for cid, _ in RUNS)
    for c in DC.CASES:
        e = X.exact_case(c)
        assert e.act == 0 and (e.ls, e.B, e.dtype, e.out) == (c.ls, c.B, c.dtype, c.out)
        assert D.case_kernels(e.ls, e.B, e.dtype, 1 if e.out else 0) == D.case_kernels(c.ls, c.B, c.dtype, 1 if c.out else 0)
        assert c.id in ran
        if c.dtype == 1:
            assert X.steps_exactly(c)
        else:                                                       # fp32: 2/B has to be an fp32 number with nothing to snap it back
            assert X.steps_exactly(c) == (c.id in X.FP32_STEP_CASES)
            assert c.id not in X.FP32_STEP_CASES or c.B & (c.B - 1) == 0
    assert all(DC.BY_ID[cid].dtype == 1 for cid in X.DROPOUT_CASES + X.SHARD_CASES)


def test_cv_comparison_is_skipped_by_logistic_cases_only():
    """At most four bf16 cases may go without the exact CV sum: they are the four with logistic columns, whose squared error is not
    exact on any data (fp32: the three logistic cases)."""
    skipped = [c.id for c in DC.CASES if X.problem(c.id).cv_sum is None]
    assert skipped == [c.id for c in DC.CASES if c.out is not None]
    assert len([cid for cid in skipped if DC.BY_ID[cid].dtype == 1]) <= 4
    for c in DC.CASES:
        p = X.problem(c.id)
        if p.cv_sum is not None:
            assert 0 < p.cv_sum < 2.0 ** 24 and p.cv_sum == int(p.cv_sum) and p.cv_skip is None


def test_targets_give_d_and_logistic_targets_never_zero():
    """dEdX_L of the handle's targets: on the linear columns o - t = d B/2 exactly; on logistic columns d != 0 and the fp32
    (2/B)(y - t), with y off by a few ulps either way, still rounds to d in bf16."""
    from torch_ref import bf16_round
    for c in X.BF16_CASES:
        p = X.problem(c.id)
        B, lin = c.B, c.ls[-1] if c.out is None else c.out[0]
        o = X.reference_outputs(p.c, p.W, p.b, p.x).astype(np.float64)
        assert np.array_equal(o[:, :lin] - p.t[:, :lin], p.d[:, :lin] * (B / 2.0))
        if c.out is None:
            continue
        assert (p.d[:, lin:] != 0).all()
        with np.errstate(over="ignore"):
            y = np.float32(1.0) / (np.float32(1.0) + np.exp(-o[:, lin:].astype(np.float32)))
        s = np.float32(2.0) / np.float32(B)
        for off in (-4, 0, 4):                                      # the device's y: a few ulps of 1.0 to either side
            yy = (y + np.float32(off * 2.0 ** -24)).astype(np.float32)
            assert np.array_equal(bf16_round(s * (yy - p.t[:, lin:])), p.d[:, lin:]), (c.id, off)


def test_todays_bar_accepts_a_dropped_frame():
    """Why this file exists.  bf_wgrad64's reference gradient with the last frame's contribution taken out of ONE 64 x 64 tile of
    G_1 -- a weight-gradient tile with a wrong k-tail -- passes the 2e-2 rms bar that tests/test_dispatch_gpu.py holds a bf16
    gradient to, and is not array_equal."""
    p, r = X.problem("bf_wgrad64"), X.reference("bf_wgrad64")
    c, B = p.c, p.c.B
    bu = X.Bunch(c, p.W, p.b, p.x[:B], p.t_oracle[:B])
    G = r.grads[0][0][1]
    assert np.array_equal(G, bu.gw[1].astype(np.float32))
    i0, j0 = 2048, 960                                              # the ragged corner tile: rows 2048 .. 2099, columns 960 .. 999
    term = np.outer(bu.ys[0][B - 1], bu.dx[1][B - 1])
    assert term[i0:i0 + 64, j0:j0 + 64].any()
    bad = G.copy()
    bad[i0:i0 + 64, j0:j0 + 64] -= term[i0:i0 + 64, j0:j0 + 64].astype(np.float32)
    err = float(np.sqrt(((bad.astype(np.float64) - G) ** 2).sum()) / np.sqrt((G.astype(np.float64) ** 2).sum()))
    print("dropped frame in one tile: relerr_rms %.3e against the bar 2e-2" % err)
    assert 0 < err < 2e-2
    assert not np.array_equal(bad, G)
    msg = X.unequal("G1", bad, G)
    assert "G1:" in msg and "worst block rows 2048.., cols 960.." in msg and "in 1 blocks of 64 x 64" in msg and "0x" in msg, msg
    assert X.count_unequal(bad, G) == int((term[i0:i0 + 64, j0:j0 + 64] != 0).sum())
    assert X.unequal("G1", G.copy(), G) is None


def test_the_checkers_notice():
    """quantum, gemm_bounds, slab_holes, zero_blocks and within_one_ulp on inputs whose answer is known."""
    assert X.quantum(np.array([0.5, 0.75, 3.0, 0.0])) == 0.25 and X.quantum(np.zeros(3)) == 1.0 and X.quantum([96.0, 64.0]) == 32.0
    rng = np.random.default_rng(3)
    A = rng.integers(1, 4, size=(70, 40)).astype(np.float64)
    Bm = rng.integers(1, 4, size=(40, 130)).astype(np.float64) * 0.25
    m, q = X.gemm_bounds(A, Bm, np.full(130, 0.125))
    assert q == 0.125 and m == (A @ Bm).max() + 0.125
    assert X.slab_holes(A, Bm) == []
    Bm[16:32, 64:128] = 0                                           # slab 1 carries no weight in column tile 1
    assert X.slab_holes(A, Bm) == [(1, 0, 1), (1, 1, 1)]
    A[64:, 32:] = 0                                                 # nor slab 2 (k = 32 .. 39) in the last block row
    assert X.slab_holes(A, Bm) == [(1, 0, 1), (1, 1, 1), (2, 1, 0), (2, 1, 1), (2, 1, 2)]
    G = np.ones((70, 130)); G[64:, 128:] = 0
    assert X.zero_blocks(G) == [(64, 128)]
    r = np.array([1.0, -3.0, 0.0], np.float32)
    assert X.within_one_ulp(r + np.spacing(r), r) and not X.within_one_ulp(r + 2 * np.spacing(np.abs(r)), r)


def test_reference_state_is_the_oracles_training_step():
    """exact_data.reference applies the oracle's update to bunch 0's gradient; the oracle's own train(), which draws the step-0
    Philox masks itself, arrives at the same words."""
    for cid, drop in (("bf_nine_layers", True), ("bf_b512", False)):
        p, r = X.problem(cid, drop), X.reference(cid, drop)
        o = X.oracle(p.c, p.W, p.b, drop=drop)
        assert o.train(p.x[:p.c.B + 3], p.t_oracle[:p.c.B + 3]) == 1
        for got, ref in zip((o.W, o.b, o.dW, o.db), r.state):
            for l in range(1, len(p.c.ls)):
                assert np.array_equal(got[l], ref[l]), (cid, l)
        assert any(o.dW[l].any() for l in range(1, len(p.c.ls)))
