"""The head of the fp32 GEMM tile program, bit for bit (-m gpu).  GemmKernel::run (csrc/bp_kernels.h) issues the loads of k-tiles 0 and 1
of a workgroup's first tile before it sets anything else up; what follows that head is, depending on the number of k-tiles, the steady
loop (three or more), the `nt - t == 2` branch (two) or the single last step (one).  A head that hands the wrong register image, stage
or k-offset to any of the three skips or doubles a k-tile, so the cases below put one, two and three (64-deep dgrad: one, three, five)
k-tiles behind it in the 32x64x64 forward and in both wide dgrad forms, run the output forward in its split and its unsplit form, and
run everything at a bunch that is a multiple of 32 and at one that is not.

Built like tests/test_exact_gpu.py: data in the recipe of tests/exact_data.py (few-bit weights, inputs and output errors), on which
every partial sum of every GEMM is an fp32 number -- the test checks that on its own data (gemm_bounds) -- so the device must give
np.array_equal to the float64 restatement of the step (exact_data.Bunch) whatever its summation order.  Held exactly: the forward
of B + 3 frames (two bunches), the stored gradient of one bunch (every G_l and bias gradient: they are made of the dgrads' results) and,
at the power-of-two bunch, one fused step from zero momentum.  The net of the split output layer is also trained on a window chunk of
two bunches in ONE call (the second bunch is stacked by the spare workgroups of the first bunch's output launch) and must then hold
the bits of two calls of one bunch each; that one is device against device, a second step is exact on no data."""
import collections

import numpy as np
import pytest

import dispatch_np as D
import exact_data as X

pytestmark = pytest.mark.gpu

Net = collections.namedtuple("Net", ["id", "ls", "dtype", "why"])
NETS = [
    # 32x64x64 forward of layer 1 (570 -> 576 columns: 9 n-tiles, the plain tile map) behind an input padded to 64, 128, 192
    Net("fwd_k64", [60, 570, 20], 0, "one k-tile: the single last step follows the head; unsplit output forward"),
    Net("fwd_k128", [100, 570, 20], 0, "two k-tiles: the nt - t == 2 branch follows the head"),
    Net("fwd_k192", [130, 570, 20], 0, "three k-tiles: the steady loop follows the head"),
    # wide dgrad of layer 2 below the 576-wide layer: 128-deep k-tiles where the padded width of layer 2 is a multiple of 128
    Net("dgrad128_k128", [60, 570, 120, 20], 0, "128-deep dgrad, one k-tile"),
    Net("dgrad128_k256", [100, 570, 250, 20], 0, "128-deep dgrad, two k-tiles"),
    Net("dgrad128_k384", [130, 570, 380, 20], 0, "128-deep dgrad, three k-tiles"),
    Net("dgrad64_k64", [60, 570, 60, 20], 0, "64-deep dgrad, one k-tile"),
    Net("dgrad64_k192", [100, 570, 190, 20], 0, "64-deep dgrad, three k-tiles"),
    Net("dgrad64_k320", [130, 570, 300, 20], 0, "64-deep dgrad, five k-tiles"),
    # 1024 columns: 16 n-tiles (the per-XCD tile map) and the output layer on the split launch
    Net("out_split", [60, 1024, 40], 0, "split output forward (4 k-slices of 4 k-tiles), 64-deep dgrad with 16 n-tiles"),
]
BUNCHES = [64, 12]
BY_ID = {n.id: n for n in NETS}
# what the shapes are there for, in the words of tests/dispatch_np.py
WIDE128, WIDE64, FWD64 = "GemmKernel<32, 64, 128, 1, 2, true, true, 2>", "GemmKernel<32, 64, 64, 1, 2, true, true, 2>", "bp_gemm<32, 64, 64, 1, 2, true, false, 0, 1>"


def test_the_nets_reach_the_kernels_they_are_named_for():
    for n in NETS:
        for B in BUNCHES:
            c = D.Config(n.ls, B)
            assert FWD64 in D.fwd_fp32(c, 1).name, n.id
            assert c.out_splits() == (D.OUT_SPLITS if n.id == "out_split" else 1), n.id
            if n.id.startswith("dgrad"):
                assert (WIDE128 if n.id.startswith("dgrad128") else WIDE64) in D.dgrad_fp32(c, 2).name, n.id
                k = c.ld[2] // (128 if n.id.startswith("dgrad128") else 64)
                assert k == {"k64": 1, "k128": 1, "k256": 2, "k384": 3, "k192": 3, "k320": 5}[n.id.split("_")[1]], n.id
    assert "bp_out_split_stage" in D.fwd_fp32(D.Config(BY_ID["out_split"].ls, 64), 2).name
    assert D.fwd_fp32(D.Config(BY_ID["fwd_k64"].ls, 64), 1).tiles_n[0] % 8 and not D.fwd_fp32(D.Config(BY_ID["out_split"].ls, 64), 1).tiles_n[0] % 8


class _Bag(object):
    pass


_DATA = {}


def _frozen(a):
    for v in (a if isinstance(a, (list, tuple)) else [a]):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a


def data(nid, B):
    """Net, B + 3 input frames, the targets of the first B and the float64 restatement, made once and read-only."""
    if (nid, B) not in _DATA:
        n, p = BY_ID[nid], _Bag()
        rng = np.random.default_rng(1000 * NETS.index(n) + B)
        vals = np.array([-2.0, -1.0, 1.0, 2.0], np.float32)
        p.n, p.W, p.b = n, [None], [None]
        for l in range(1, len(n.ls)):
            prev, cur = n.ls[l - 1], n.ls[l]
            nz = X.weight_pattern(rng, prev, cur)
            p.W.append(np.where(nz, rng.choice(vals, size=(prev, cur)), np.float32(0.0)).astype(np.float32))
            p.b.append((rng.integers(-2, 3, size=cur) * 0.5).astype(np.float32))
        p.x = (rng.integers(-3, 4, size=(B + 3, n.ls[0])) * 0.5).astype(np.float32)
        p.forward = X.Bunch(n, p.W, p.b, p.x, np.zeros((B + 3, n.ls[-1]), np.float32)).out.astype(np.float32)
        p.d = X.D_VALUES[rng.integers(0, len(X.D_VALUES), size=(B, n.ls[-1]))]
        t = p.forward[:B].astype(np.float64) - p.d * (B / 2.0)
        p.t = t.astype(np.float32)
        assert np.array_equal(p.t.astype(np.float64), t), (nid, B, "the targets are no fp32 numbers")
        p.bunch = bu = X.Bunch(n, p.W, p.b, p.x[:B], p.t)
        # the conditions of exact_data on THIS data: (2/B)(o - t) rounds to d (a d of two significant bits absorbs the one-ulp
        # error of 2/12), and every GEMM of the step accumulates exactly
        assert np.array_equal(bu.dx[len(n.ls) - 1], p.d), (nid, B, "dEdX_L is not d")
        for name, A, Bm, add in bu.gemms:
            m, q = X.gemm_bounds(A, Bm, add)
            assert m / q < 2.0 ** 24 and q >= 2.0 ** -40, (nid, B, name, m, q)
        # one fused step from zero momentum, lr 0.5, momentum 0.5, no weight cost: dW = -1/4 G / B, W' = W + dW; exact where B is
        # a power of two (asserted: every value an fp32 number)
        p.step = None
        if B & (B - 1) == 0:
            p.step = [[None], [None], [None], [None]]
            for l in range(1, len(n.ls)):
                for k, (g, w) in enumerate(((bu.gw[l], p.W[l]), (bu.gb[l], p.b[l]))):
                    dw = -0.25 * g / B
                    wn = w.astype(np.float64) + dw
                    assert np.array_equal(dw.astype(np.float32).astype(np.float64), dw) and np.array_equal(wn.astype(np.float32).astype(np.float64), wn), (nid, B, l)
                    p.step[k].append(wn.astype(np.float32))
                    p.step[2 + k].append(dw.astype(np.float32))
        _frozen(p.W[1:] + p.b[1:] + [p.x, p.t, p.forward] + bu.gw[1:] + bu.gb[1:] + ([] if p.step is None else [a for s in p.step for a in s[1:]]))
        _DATA[(nid, B)] = p
    return _DATA[(nid, B)]


def _mk(pkg, p, B, cap):
    return pkg.BP_GPU(1, len(p.n.ls), p.n.ls, B, X.LR, X.MOM, X.WC, p.W, p.b, activation=0, compute_dtype=0, max_chunk_frames=cap)


CASES = [(n.id, B) for n in NETS for B in BUNCHES]
_ids = ["%s-b%d" % c for c in CASES]


@pytest.mark.parametrize("nid,B", CASES, ids=_ids)
def test_forward_is_exact(pkg, nid, B):
    p = data(nid, B)
    g = _mk(pkg, p, B, 2 * B)
    out = g.forward(p.x)
    g.close()
    msg = X.unequal("forward of %d frames" % p.x.shape[0], out, p.forward)
    print(nid, B, "forward, unequal elements:", X.count_unequal(out, p.forward))
    assert msg is None, (nid, B, msg)


@pytest.mark.parametrize("nid,B", CASES, ids=_ids)
def test_gradient_is_exact(pkg, nid, B):
    """grads_resident on one bunch: G_l = y_{l-1}^T dEdX_l for every layer, so every dgrad's result is in it."""
    p = data(nid, B)
    g = _mk(pkg, p, B, 2 * B)
    g.upload_chunk(p.x[:B], p.t)
    g.grads_resident(0)
    gw, gb = g.read_grads()
    g.close()
    fails, counts = [], {}
    for l in range(1, len(p.n.ls)):
        for name, a, r in (("G%d" % l, gw[l], p.bunch.gw[l]), ("gb%d" % l, gb[l], p.bunch.gb[l])):
            a = np.asarray(a, np.float32).reshape(np.asarray(r).shape)
            counts[name] = X.count_unequal(a, r)
            msg = X.unequal(name, a, r)
            if msg:
                fails.append(msg)
    print(nid, B, "gradient, unequal elements:", counts)
    assert not fails, (nid, B, fails)


STEP_CASES = [(nid, B) for nid, B in CASES if B & (B - 1) == 0]


@pytest.mark.parametrize("nid,B", STEP_CASES, ids=["%s-b%d" % c for c in STEP_CASES])
def test_fused_step_is_exact(pkg, nid, B):
    p = data(nid, B)
    g = _mk(pkg, p, B, B)
    g.train(B, p.x[:B], p.t)
    got = g.get_weights() + g.get_deltas()
    g.close()
    fails, counts = [], {}
    for i, nm in enumerate(("W", "b", "dW", "db")):
        for l in range(1, len(p.n.ls)):
            name = "%s%d" % (nm, l)
            counts[name] = X.count_unequal(got[i][l], p.step[i][l])
            msg = X.unequal(name, got[i][l], p.step[i][l])
            if msg:
                fails.append(msg)
    print(nid, B, "fused step, unequal elements:", counts)
    assert not fails, (nid, B, fails)


@pytest.mark.parametrize("B", BUNCHES)
def test_two_bunches_in_one_call_are_two_calls_of_one(pkg, B):
    """A window chunk of 2 B samples trained in one call -- the second bunch is stacked into the other staged tile by the spare
    workgroups of the first bunch's output launch (bp_out_split_stage) -- against the same samples in two calls of B."""
    p = data("out_split", B)
    fea_dim, context = 20, 3
    assert fea_dim * context == p.n.ls[0]
    rng = np.random.default_rng(7 + B)
    fea = (rng.integers(-3, 4, size=(2 * B + context, fea_dim)) * 0.5).astype(np.float32)
    targ = (rng.integers(-4, 5, size=(2 * B + context, p.n.ls[-1])) * 0.5).astype(np.float32)
    ws = np.arange(2 * B, dtype=np.int32)
    tf = ws + 1
    states = []
    for cuts in ([slice(0, 2 * B)], [slice(0, B), slice(B, 2 * B)]):
        g = _mk(pkg, p, B, 2 * B)
        for s in cuts:
            g.train_windows(fea, targ, context, ws[s], tf[s])
        states.append(g.get_weights() + g.get_deltas())
        g.close()
    fails = []
    for i, nm in enumerate(("W", "b", "dW", "db")):
        for l in range(1, len(p.n.ls)):
            msg = X.unequal("%s%d, one call against two" % (nm, l), states[0][i][l], states[1][i][l])
            if msg:
                fails.append(msg)
            assert np.isfinite(states[0][i][l]).all() and np.any(states[0][i][l] != (p.W, p.b)[i][l] if i < 2 else states[0][i][l] != 0), (nm, l)
    assert not fails, (B, fails)
