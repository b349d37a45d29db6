"""The persistent weight-gradient launch (bp_wgrad_dma.h, -m gpu): a workgroup walks several tiles and keeps the operand loads of
its next tile in flight across the tile boundary.  The nets of a test have fewer tiles than the launch has slots, so each case
builds two handles from the same weights and seed: BP_WGRAD_SLOTS=8 (read at handle creation: eight workgroups, every one walks
many tiles, across the problems of the grouped launch) and a slot count above the tile count (one tile per workgroup: only the
first-tile path runs).  Three training bunches; W, b, delta W and delta b must be the same bits -- the walk changes which
workgroup computes a tile, never the arithmetic of one.  One case per bunch size is also held against the oracle at util.TOL.

Seams and the smallest shapes that reach them:
  problem boundary inside a walk, plain tile map, ragged widths      [130, 192, 257]            B 128
  XCD tile map (tiles_n % 8 == 0) followed by a narrow problem       [192, 512, 257]            B 256
  32 k-tiles per tile                                                [130, 192, 257]            B 512
  bias tile directly followed by another tile of the workgroup       every case (8 slots)
  second grouped launch (more than 4 weight layers)                  six layers, widths 130-192 B 128
  gradient-store form (grads_resident) and its tile counters         both nets                  B 128, B 256
The tile counters are only read by the exchange kernels of an attached group: a one-rank group trains through them, and a layer
whose counter stopped short of its tile count would leave the exchange waiting until BP_DP_TIMEOUT_S and fail the call.
The last test holds the other direction too: which handles report the in-kernel hand-off, and that each trains right."""
import os

import numpy as np
import pytest

from util import TOL, relerr

pytestmark = pytest.mark.gpu

FEW, MANY = 8, 1 << 20
NET_PLAIN, NET_XCD = [130, 192, 257], [192, 512, 257]
NET_DEEP = [130, 192, 160, 130, 192, 150, 257]
DROP = dict(dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=7)


def _data(ls, n, seed):
    from oracle import bp_numpy as N
    W, b = N.glorot_net(ls, seed=seed, beta=0.5)
    rng = np.random.default_rng(seed + 100)
    return W, b, rng.normal(size=(n, ls[0])).astype(np.float32), rng.normal(size=(n, ls[-1])).astype(np.float32)


def _handle(pkg, slots, ls, B, W, b, cap, kw):
    os.environ["BP_WGRAD_SLOTS"] = str(slots)
    try:
        return pkg.BP_GPU(1, len(ls), ls, B, 1.0, 0.5, 0.0, W, b, max_chunk_frames=cap, **kw)
    finally:
        del os.environ["BP_WGRAD_SLOTS"]


def _trained(pkg, slots, ls, B, W, b, x, t, kw, attach=None):
    g = _handle(pkg, slots, ls, B, W, b, x.shape[0], kw)
    if attach:
        g.dp_attach(1, 0, "%s-%d-%d" % (attach, os.getpid(), slots))
        assert g.dp_handoff() is True, "the tile-counting launch is what this case is about"
    g.train(x.shape[0], x, t)
    state = g.get_weights() + g.get_deltas()
    if attach:
        g.dp_detach()
    g.close()
    return state


def _same_bits(ls, few, many, names=("W", "b", "dW", "db")):
    for k, name in enumerate(names):
        for l in range(1, len(ls)):
            a, r = np.asarray(few[k][l]), np.asarray(many[k][l])
            assert a.any(), (name, l, "all zero")
            assert np.array_equal(a, r), ("%s%d differs between 8 slots and one tile per workgroup" % (name, l),
                                         int((a != r).sum()), "words; first at", np.argwhere(a != r)[:4].tolist())


@pytest.mark.parametrize("ls,B,kw,oracle", [
    (NET_PLAIN, 128, DROP, True),
    (NET_XCD, 256, {}, True),
    (NET_PLAIN, 512, {}, True),
    (NET_DEEP, 128, DROP, False),
], ids=["plain_b128_dropout", "xcd_b256", "plain_b512", "six_layers_b128_dropout"])
def test_fused_walk_is_bit_identical(pkg, oracle_mod, ls, B, kw, oracle):
    W, b, x, t = _data(ls, 3 * B, seed=B + len(ls))
    few = _trained(pkg, FEW, ls, B, W, b, x, t, kw)
    many = _trained(pkg, MANY, ls, B, W, b, x, t, kw)
    _same_bits(ls, few, many)
    if oracle:
        o = oracle_mod.Oracle(ls, B, 1.0, 0.5, 0.0, W, b, **kw)
        o.train(x, t)
        errs = {}
        for k, (name, ref) in enumerate((("W", o.W), ("b", o.b), ("dW", o.dW), ("db", o.db))):
            for l in range(1, len(ls)):
                errs["%s%d" % (name, l)] = relerr(few[k][l], ref[l])
        print(ls, B, errs)
        assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("ls,B", [(NET_PLAIN, 128), (NET_XCD, 256)], ids=["plain_b128", "xcd_b256"])
def test_store_walk_is_bit_identical(pkg, ls, B):
    """The stored gradient of one bunch (grads_resident, the call of tests/test_dispatch_gpu.py), pad rows and columns included."""
    W, b, x, t = _data(ls, B, seed=B + 1)
    got = []
    for slots in (FEW, MANY):
        g = _handle(pkg, slots, ls, B, W, b, B, {})
        g.upload_chunk(x, t)
        g.grads_resident(0)
        got.append(g.read_grads(padded=True))
        g.close()
    _same_bits(ls, got[0], got[1], names=("G", "gb"))


@pytest.mark.parametrize("ls,B,kw", [(NET_PLAIN, 128, DROP), (NET_XCD, 256, {})], ids=["plain_b128_dropout", "xcd_b256"])
def test_store_walk_counts_every_tile(pkg, ls, B, kw):
    """A one-rank group: the store form with its per-layer tile counters, which the exchange waits for."""
    W, b, x, t = _data(ls, 3 * B, seed=B + 2)
    few = _trained(pkg, FEW, ls, B, W, b, x, t, kw, attach="walk")
    many = _trained(pkg, MANY, ls, B, W, b, x, t, kw, attach="walk")
    _same_bits(ls, few, many)


@pytest.mark.parametrize("ls,B,dtype,handoff", [
    (NET_PLAIN, 512, 0, True),
    (NET_PLAIN, 1024, 0, False),
    (NET_DEEP, 128, 0, False),
    (NET_PLAIN, 128, 1, False),
], ids=["fp32_b512", "fp32_b1024_bf16_only_size", "fp32_six_weight_layers", "bf16_b128"])
def test_handoff_follows_the_kernel_that_counts(pkg, oracle_mod, ls, B, dtype, handoff):
    """The exchange waits on tile counters exactly when the launch it runs beside bumps them (fp32 store kernel of a static bunch
    size, at most four weight layers).  A one-rank group, three bunches, against the oracle: a handle that claims the hand-off
    without the counting kernel times out in the exchange, one that counts unasked or takes the wrong kernel misses the oracle.
    Bars: fp32 util.TOL (the oracle's own fp32 / fp64-accumulation spread on these nets, bunches and seeds is at most 7.5e-7);
    bf16 those of test_dispatch_gpu (W, b at TOL_BF16 / 4, momentum state 2e-2 rms; rate 0.5)."""
    from test_dispatch_gpu import LR, TOL_BF16, relerr_rms
    W, b, x, t = _data(ls, 3 * B, seed=B + 3)
    g = pkg.BP_GPU(1, len(ls), ls, B, LR[dtype], 0.5, 0.0, W, b, max_chunk_frames=3 * B, compute_dtype=dtype)
    g.dp_attach(1, 0, "handoff-%d-%d-%d-%d" % (os.getpid(), len(ls), B, dtype))
    assert g.dp_handoff() is handoff
    g.train(3 * B, x, t)
    got = g.get_weights() + g.get_deltas()
    g.dp_detach()
    g.close()
    o = oracle_mod.Oracle(ls, B, LR[dtype], 0.5, 0.0, W, b, compute_dtype=dtype)
    o.train(x, t)
    errs, fails = {}, []
    for k, (name, ref) in enumerate((("W", o.W), ("b", o.b), ("dW", o.dW), ("db", o.db))):
        for l in range(1, len(ls)):
            if dtype == 0:
                e, bar = relerr(got[k][l], ref[l]), TOL
            elif k < 2:
                e, bar = relerr(got[k][l], ref[l]), TOL_BF16 / 4
            else:
                e, bar = relerr_rms(got[k][l], ref[l]), TOL_BF16
            errs["%s%d" % (name, l)] = e
            if not e < bar:
                fails.append(("%s%d" % (name, l), e, bar))
    print(ls, B, dtype, errs)
    assert not fails, fails
