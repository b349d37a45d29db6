"""Every path of the fp32 k-loops of the wide forward and the 128-deep dgrad, bit for bit (-m gpu): GemmKernel::run
(csrc/bp_kernels.h) walks a workgroup's k-tiles through a head, a steady-state loop unrolled by two and one or two tail steps, so
the number of k-tiles decides which of them run and which LDS stage and register image the last tile comes from.

The nets are [64 n, 576, 64 n, 576, 40] for n = 1 .. 6.  Layer 1 (64 n -> 576) is the wide forward as input layer and layer 3 the
wide forward as hidden layer, each with n k-tiles of 64: one tile; two (head and one tail step); three .. six (the loop once or
twice, with an odd and an even rest).  The dgrad of layer 2 (dEdX_1 [B][576] from dEdX_2 [B][64 n]) is the 128-deep one for even n,
with cur = 128, 256 and 384: its first k-tile is the last, a loop-free pair, and an odd count.  tests/dispatch_np.py is asked
that each net reaches the kernel it is meant for.

The data is that of tests/exact_data.py (few-bit weights, inputs and output errors): every partial sum of every GEMM is an fp32
number -- asserted on the data (gemm_bounds) -- so the device must be np.array_equal to the float64 restatement in any summation
order: a k that is skipped or taken twice, or a stage read while it is being overwritten, is a different number.  Bunches of 1,
33 and 64 frames, hidden dropout off and at 0.5: inference (forward) and one fused step; at 33 frames, where the step size
lr 2/33 is no fp32 number and the updated weights are not exact, the stored gradient of the same bunch stands for the step
(the forward, every dgrad and the weight-gradient GEMMs are the step's)."""
import numpy as np
import pytest

import dispatch_cases as DC
import dispatch_np as D
import exact_data as X
import philox_np as P

gpu = pytest.mark.gpu

NS = [1, 2, 3, 4, 5, 6]
BUNCHES = [1, 33, 64]
SEED = 0x9E3779B97F4A7C15
HID_OMIT = 0.5

WIDE_FWD = "bp_gemm<32, 64, 64, 1, 2, true, false, 0, %d>"
NARROW_FWD = "bp_gemm<32, 32, 64, 1, 1, true, false, 0, 0>"
WIDE64_DG, WIDE128_DG = "GemmKernel<32, 64, 64, 1, 2, true, true, 2>", "GemmKernel<32, 64, 128, 1, 2, true, true, 2>"


def layers(n):
    return [64 * n, 576, 64 * n, 576, 40]


def test_the_nets_reach_the_kernels_they_are_named_for():
    for n in NS:
        for B in BUNCHES:
            c = D.Config(layers(n), B)
            assert c.ld[:4] == [64 * n, 576, 64 * n, 576]                    # k-tiles of 64: n in layer 1 and in layer 3
            assert WIDE_FWD % 1 in D.fwd_fp32(c, 1).name and WIDE_FWD % 0 in D.fwd_fp32(c, 3).name
            assert NARROW_FWD in D.fwd_fp32(c, 2).name
            assert (WIDE128_DG if n % 2 == 0 else WIDE64_DG) in D.dgrad_fp32(c, 2).name     # K = 64 n: one, two, three 128-deep tiles
            assert WIDE64_DG in D.dgrad_fp32(c, 4).name


class _Bag(object):
    pass


_DATA = {}


def _net(c, n):
    """exact_data.net with a seed of this file's (that one takes its seed from the case table)."""
    rng = np.random.default_rng(7000 + n)
    vals = X.weight_values(c)
    W, b = [None], [None]
    for l in range(1, len(c.ls)):
        prev, cur = c.ls[l - 1], c.ls[l]
        nz = X.weight_pattern(rng, prev, cur)
        W.append(np.where(nz, rng.choice(vals, size=(prev, cur)), np.float32(0.0)).astype(np.float32))
        b.append((rng.integers(-2, 3, size=cur) * 0.5).astype(np.float32))
    return W, b


def data(n, B, drop):
    """Net, B + 3 input frames, targets of the first B and the float64 restatement of one bunch (exact_data.Bunch), made once and
    read-only.  drop: hidden dropout HID_OMIT with the masks of step 0 (philox_np.drop_mask; the input layer keeps everything)."""
    if (n, B, drop) not in _DATA:
        c = DC.Case("kloop_n%d" % n, layers(n), B, 0, 0, None, None, "k-loop paths")
        p, L = _Bag(), 5
        p.c = c
        p.W, p.b = _net(c, n)
        p.x = (np.random.default_rng(7100 + n).integers(-3, 4, size=(B + 3, c.ls[0])) * 0.5).astype(np.float32)
        p.mk = None
        if drop:
            p.mk = [np.zeros((B, c.ls[0]), np.uint8)] + [P.drop_mask(SEED, 0, l, B, c.ls[l], HID_OMIT, 0) for l in range(1, L - 1)]
        p.forward = X.Bunch(c, p.W, p.b, p.x, np.zeros((B + 3, c.ls[-1]), np.float32)).out.astype(np.float32)      # inference: no mask
        out = X.Bunch(c, p.W, p.b, p.x[:B], np.zeros((B, c.ls[-1]), np.float32), p.mk).out
        rng = np.random.default_rng(7200 + 100 * n + B + (1000 if drop else 0))
        p.d = X.D_VALUES[rng.integers(0, len(X.D_VALUES), size=(B, c.ls[-1]))]
        t = out - p.d * (B / 2.0)
        p.t = t.astype(np.float32)
        assert np.array_equal(p.t.astype(np.float64), t), (n, B, "the targets are no fp32 numbers")
        p.bunch = bu = X.Bunch(c, p.W, p.b, p.x[:B], p.t, p.mk)
        assert np.array_equal(bu.dx[L - 1], p.d), (n, B, "dEdX_L is not d")
        for name, A, Bm, add in bu.gemms:
            m, q = X.gemm_bounds(A, Bm, add)
            assert m / q < 2.0 ** 24 and q >= 2.0 ** -40, (n, B, name, m, q)
        # one fused step from zero momentum, lr 0.5, momentum 0.5, no weight cost: dW = -1/4 G / B, W' = W + dW; exact where B is a
        # power of two (asserted: every value an fp32 number)
        p.step = None
        if B & (B - 1) == 0:
            p.step = [[None], [None], [None], [None]]
            for l in range(1, L):
                for k, (g, w) in enumerate(((bu.gw[l], p.W[l]), (bu.gb[l], p.b[l]))):
                    dw = -0.25 * g / B
                    wn = w.astype(np.float64) + dw
                    assert np.array_equal(dw.astype(np.float32).astype(np.float64), dw) and np.array_equal(wn.astype(np.float32).astype(np.float64), wn), (n, B, l)
                    p.step[k].append(wn.astype(np.float32))
                    p.step[2 + k].append(dw.astype(np.float32))
        for a in p.W[1:] + p.b[1:] + [p.x, p.t, p.forward] + bu.gw[1:] + bu.gb[1:] + ([] if p.step is None else [a for s in p.step for a in s[1:]]):
            a.setflags(write=False)
        _DATA[(n, B, drop)] = p
    return _DATA[(n, B, drop)]


def test_the_data_is_exact_and_sees_every_k_tile():
    """No GPU: condition (a) of exact_data on every GEMM of every case (asserted in data()), and every 16-wide slab of the reduction
    of the forwards of layers 1 and 3 and of the dgrad of layer 2 reaches every 64 x 64 output block: a k-tile cannot go missing
    unseen.  (One-frame bunches: a block row of one frame meets one weight row per slab; the 33- and 64-frame bunches carry that.)"""
    for n in NS:
        for B in BUNCHES:
            for drop in (False, True):
                p = data(n, B, drop)
                if B >= 33 and not drop:
                    for name, A, Bm, _ in p.bunch.gemms:
                        if name in ("forward 1", "forward 3", "dgrad 2"):
                            assert X.slab_holes(A, Bm) == [], (n, B, name)


def _mk(pkg, p, B, cap, drop):
    kw = dict(activation=0, compute_dtype=0, max_chunk_frames=cap)
    if drop:
        kw.update(dropoutflag=1, visible_omit=0.0, hid_omit=HID_OMIT, seed=SEED)
    return pkg.BP_GPU(1, len(p.c.ls), p.c.ls, B, X.LR, X.MOM, X.WC, p.W, p.b, **kw)


CASES = [(n, B, drop) for n in NS for B in BUNCHES for drop in (False, True)]


@gpu
@pytest.mark.parametrize("n,B,drop", CASES, ids=["n%d-b%d-%s" % (n, B, "drop" if d else "keep") for n, B, d in CASES])
def test_every_k_loop_path(pkg, n, B, drop):
    p = data(n, B, drop)
    fails = []
    if not drop:                                  # inference draws nothing: once per net and bunch
        g = _mk(pkg, p, B, B + 3, False)
        out = g.forward(p.x)
        g.close()
        print(n, B, "forward, unequal elements:", X.count_unequal(out, p.forward))
        msg = X.unequal("forward of %d frames" % p.x.shape[0], out, p.forward)
        if msg:
            fails.append(msg)
    g = _mk(pkg, p, B, 2 * B, drop)
    counts = {}
    if p.step is not None:
        g.train(B, p.x[:B], p.t)
        got = g.get_weights() + g.get_deltas()
        for i, nm in enumerate(("W", "b", "dW", "db")):
            for l in range(1, len(p.c.ls)):
                counts["%s%d" % (nm, l)] = X.count_unequal(got[i][l], p.step[i][l])
                msg = X.unequal("%s%d" % (nm, l), got[i][l], p.step[i][l])
                if msg:
                    fails.append(msg)
    else:
        g.upload_chunk(p.x[:B], p.t)
        g.grads_resident(0)
        gw, gb = g.read_grads()
        for l in range(1, len(p.c.ls)):
            for name, a, r in (("G%d" % l, gw[l], p.bunch.gw[l]), ("gb%d" % l, gb[l], p.bunch.gb[l])):
                a = np.asarray(a, np.float32).reshape(np.asarray(r).shape)
                counts[name] = X.count_unequal(a, r)
                msg = X.unequal(name, a, r)
                if msg:
                    fails.append(msg)
    g.close()
    print(n, B, drop, "fused step" if p.step is not None else "stored gradient", "unequal elements:", counts)
    assert not fails, (n, B, drop, fails)
