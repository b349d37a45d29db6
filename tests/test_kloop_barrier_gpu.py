"""The k-tile barrier of the fp32 GEMMs where tests/test_kloop_paths_gpu.py does not reach, bit for bit and over and over (-m gpu).
GemmCfg::step (csrc/bp_kernels.h) carries the k-tile's barrier and, behind it, reads the first fragments of the next tile from the
other LDS stage; in the forwards the barrier stands in front of the tile's last MFMA.  A stage read before it is whole, or
overwritten while a wave still reads it, is a different number on the data of tests/exact_data.py (every partial sum of every GEMM an
fp32 number, asserted on the data: the device must be np.array_equal to the float64 restatement in any order), but only when the
waves happen to be far enough apart: so every case runs 25 times on one handle, each repetition compared.

 - Nets [64 n, 64, 64 n, 64, 40], n = 1 .. 5: layers 1 and 3 are the narrow forward bp_gemm<32, 32, 64, 1, 1, ...> (four wave groups
   split each k-tile, eight MFMA steps each) with n k-tiles, and the dgrad of layer 2 the narrow dgrad with n k-tiles: one tile;
   a loop-free pair; the loop once and twice, with an odd and an even rest.
 - Nets [64, H, 40], H = 1024, 1280, 1536: the one-launch output forward bp_out_split_stage with 4, 5 and 6 k-tiles per k-slice.
   A handle takes that kernel from a 1024-wide last hidden layer on (bp_create), so four tiles per slice are the fewest it can
   be given: the loop once with a pair behind it, twice with one tile, twice with a pair.
 - Bunches of 33 frames (a partial block of rows) and of 256 (eight m-tile workgroups per weight panel, as in training).

Each repetition is an inference forward of B + 3 frames and the stored gradient of one bunch (upload_chunk, grads_resident,
read_grads: the forward, every dgrad and the weight-gradient GEMMs of the step; none of them changes the handle's weights).
tests/dispatch_np.py is asked that each net reaches the kernel it is named for."""
import numpy as np
import pytest

import dispatch_cases as DC
import dispatch_np as D
import exact_data as X

gpu = pytest.mark.gpu

NS = [1, 2, 3, 4, 5]
HS = [1024, 1280, 1536]
BUNCHES = [33, 256]
REPS = 25

NARROW_FWD = "bp_gemm<32, 32, 64, 1, 1, true, false, 0, 0>"
NARROW_DG = "GemmKernel<32, 32, 64, 1, 1, true, true, 2>"
OUT_SPLIT = "bp_out_split_stage<GemmKernel<32, 32, 64, 1, 1, true, false, 6> >"


def narrow(n):
    return [64 * n, 64, 64 * n, 64, 40]


def split(H):
    return [64, H, 40]


NETS = [("narrow%d" % n, narrow(n)) for n in NS] + [("split%d" % H, split(H)) for H in HS]


def test_the_nets_reach_the_kernels_they_are_named_for():
    for B in BUNCHES:
        for n in NS:
            c = D.Config(narrow(n), B)
            assert c.ld[:4] == [64 * n, 64, 64 * n, 64]                      # k-tiles of 64: n in layers 1 and 3 and in dgrad 2
            assert NARROW_FWD in D.fwd_fp32(c, 1).name and NARROW_FWD in D.fwd_fp32(c, 2).name and NARROW_FWD in D.fwd_fp32(c, 3).name
            assert NARROW_DG in D.dgrad_fp32(c, 2).name and NARROW_DG in D.dgrad_fp32(c, 3).name
        for H in HS:
            c = D.Config(split(H), B)
            # 1, 2 or 3 k-tiles per slice would need a last hidden layer of 256, 512 or 768: below 1024 bp_create leaves the output
            # layer unsplit (out_splits() == 1) and the narrow bp_gemm takes it, whose step -- the same GemmCfg<32, 32, 64, 1, 1, true,
            # false> -- the nets above run at 1 .. 5 tiles.  4 is the fewest this kernel is ever launched with.
            assert all(D.Config(split(h), B).out_splits() == 1 for h in (256, 512, 768))
            assert c.out_splits() == D.OUT_SPLITS == 4 and c.ld[1] == H and H // D.OUT_SPLITS // 64 in (4, 5, 6)
            assert OUT_SPLIT in D.fwd_fp32(c, 2).name


class _Bag(object):
    pass


_DATA = {}


def data(name, ls, B):
    """Net, B + 3 input frames, targets of the first B and the float64 restatement of one bunch (exact_data.Bunch), made once and
    read-only.  Condition (a) of exact_data is asserted on every GEMM."""
    if (name, B) not in _DATA:
        c = DC.Case("kbar_%s" % name, ls, B, 0, 0, None, None, "k-tile barrier")
        p, L = _Bag(), len(ls)
        seed = 9000 + 16 * [k for k, _ in NETS].index(name)
        p.c = c
        rng = np.random.default_rng(seed)
        vals = X.weight_values(c)
        p.W, p.b = [None], [None]
        for l in range(1, L):
            prev, cur = ls[l - 1], ls[l]
            nz = X.weight_pattern(rng, prev, cur)
            p.W.append(np.where(nz, rng.choice(vals, size=(prev, cur)), np.float32(0.0)).astype(np.float32))
            p.b.append((rng.integers(-2, 3, size=cur) * 0.5).astype(np.float32))
        p.x = (np.random.default_rng(seed + 1).integers(-3, 4, size=(B + 3, ls[0])) * 0.5).astype(np.float32)
        p.forward = X.Bunch(c, p.W, p.b, p.x, np.zeros((B + 3, ls[-1]), np.float32)).out.astype(np.float32)
        out = X.Bunch(c, p.W, p.b, p.x[:B], np.zeros((B, ls[-1]), np.float32)).out
        p.d = X.D_VALUES[np.random.default_rng(seed + 2 + B).integers(0, len(X.D_VALUES), size=(B, ls[-1]))]
        t = out - p.d * (B / 2.0)
        p.t = t.astype(np.float32)
        assert np.array_equal(p.t.astype(np.float64), t), (name, B, "the targets are no fp32 numbers")
        p.bunch = bu = X.Bunch(c, p.W, p.b, p.x[:B], p.t)
        assert np.array_equal(bu.dx[L - 1], p.d), (name, B, "dEdX_L is not d")
        for gname, A, Bm, add in bu.gemms:
            m, q = X.gemm_bounds(A, Bm, add)
            assert m / q < 2.0 ** 24 and q >= 2.0 ** -40, (name, B, gname, m, q)
        p.gw = [None] + [g.astype(np.float32) for g in bu.gw[1:]]
        p.gb = [None] + [g.astype(np.float32) for g in bu.gb[1:]]
        for l in range(1, L):
            assert np.array_equal(p.gw[l].astype(np.float64), bu.gw[l]) and np.array_equal(p.gb[l].astype(np.float64), bu.gb[l]), (name, B, l)
        for a in p.W[1:] + p.b[1:] + [p.x, p.t, p.forward] + p.gw[1:] + p.gb[1:]:
            a.setflags(write=False)
        _DATA[(name, B)] = p
    return _DATA[(name, B)]


def test_the_data_is_exact_and_sees_every_k_tile():
    """No GPU: condition (a) on every GEMM of every case (asserted in data()), and every 16-wide slab of the reduction of every
    forward and dgrad reaches every 64 x 64 output block: a k-tile, or a wave group's quarter of one, cannot go missing unseen."""
    for name, ls in NETS:
        for B in BUNCHES:
            p = data(name, ls, B)
            for gname, A, Bm, _ in p.bunch.gemms:
                if gname.startswith("forward") or gname.startswith("dgrad"):
                    assert X.slab_holes(A, Bm) == [], (name, B, gname)


CASES = [(name, ls, B) for name, ls in NETS for B in BUNCHES]


@gpu
@pytest.mark.parametrize("name,ls,B", CASES, ids=["%s-b%d" % (name, B) for name, _, B in CASES])
def test_every_repetition_is_the_exact_result(pkg, name, ls, B):
    p = data(name, ls, B)
    g = pkg.BP_GPU(1, len(ls), ls, B, X.LR, X.MOM, X.WC, p.W, p.b, activation=0, compute_dtype=0, max_chunk_frames=2 * B)
    fails, counts = [], {}
    try:
        for rep in range(REPS):
            out = g.forward(p.x)
            n = X.count_unequal(out, p.forward)
            if n:
                counts[(rep, "forward")] = n
                fails.append("repetition %d: %s" % (rep, X.unequal("forward of %d frames" % p.x.shape[0], out, p.forward)))
            g.upload_chunk(p.x[:B], p.t)
            g.grads_resident(0)
            gw, gb = g.read_grads()
            for l in range(1, len(ls)):
                for what, a, r in (("G%d" % l, gw[l], p.gw[l]), ("gb%d" % l, gb[l], p.gb[l])):
                    a = np.asarray(a, np.float32).reshape(r.shape)
                    n = X.count_unequal(a, r)
                    if n:
                        counts[(rep, what)] = n
                        fails.append("repetition %d: %s" % (rep, X.unequal(what, a, r)))
    finally:
        g.close()
    print(name, B, "%d repetitions, unequal elements:" % REPS, counts)
    assert not fails, (name, B, len(fails), fails[:4])
