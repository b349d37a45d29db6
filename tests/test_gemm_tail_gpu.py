"""The tail of the fp32 GEMM tile program, bit for bit (-m gpu): what GemmKernel::run (csrc/bp_kernels.h) does behind its last MFMA.
The hidden forward draws its dropout words there (drop_words4 / philox4x32_10, csrc/bp_device.h); the hidden forward and the dgrad
store a 32 x 32 block that lies wholly inside the bunch through a uniform row base and a partial block row by row (block_store);
and a workgroup computes ONE tile, which the host checks in front of every launch (covers_tiles).

The nets are those of tests/dispatch_cases.py that reach the narrow forward and dgrad (32 x 32 tiles, four waves share a block: KS =
4), the wide ones (32 x 64 tiles, KS = 2; 64-deep dgrad), the 128-deep dgrad and the split output launch, run at the bunch sizes
this file needs, on the data of tests/exact_data.py (few-bit weights, inputs and output errors): every partial sum of every GEMM is
an fp32 number -- checked here on the data itself (gemm_bounds) -- so the device must be np.array_equal to the float64 restatement
of the step (exact_data.Bunch) with the masks of tests/philox_np.py, whatever its summation order."""
import os
import subprocess

import numpy as np
import pytest

import dispatch_cases as DC
import dispatch_np as D
import exact_data as X
import philox_np as P

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

NETS = ["f32_xcd_narrow", "f32_wide_hidden", "f32_wide128_ragged"]
SEED = 0xF00DFACE8BADF00D          # high bits set in both 32-bit halves of the key
HID_OMIT = 0.5
OFFSETS = [0, 1, 2, 3]             # frame_off & 3: one Philox block per four rows, or the three ways four rows straddle two
BUNCHES = [1, 31, 33, 64]          # no whole block | one partial | one whole + one partial | two whole 32-row blocks

NARROW_FWD, WIDE_FWD = "bp_gemm<32, 32, 64, 1, 1, true, false, 0, 0>", "bp_gemm<32, 64, 64, 1, 2, true, false, 0, 1>"
NARROW_DG, WIDE64_DG, WIDE128_DG = ("GemmKernel<32, 32, 64, 1, 1, true, true, 2>", "GemmKernel<32, 64, 64, 1, 2, true, true, 2>",
                                    "GemmKernel<32, 64, 128, 1, 2, true, true, 2>")


def test_the_nets_reach_the_kernels_they_are_named_for():
    for B in BUNCHES:
        c = D.Config(DC.BY_ID["f32_xcd_narrow"].ls, B)
        assert NARROW_FWD in D.fwd_fp32(c, 1).name and NARROW_FWD in D.fwd_fp32(c, 2).name and NARROW_DG in D.dgrad_fp32(c, 2).name
        c = D.Config(DC.BY_ID["f32_wide_hidden"].ls, B)
        assert WIDE_FWD in D.fwd_fp32(c, 1).name and WIDE_FWD[:-3] in D.fwd_fp32(c, 2).name and WIDE64_DG in D.dgrad_fp32(c, 2).name
        c = D.Config(DC.BY_ID["f32_wide128_ragged"].ls, B)
        assert WIDE128_DG in D.dgrad_fp32(c, 2).name and c.out_splits() == D.OUT_SPLITS and "bp_out_split_stage" in D.fwd_fp32(c, 3).name


class _Bag(object):
    pass


_DATA = {}


def _frozen(a):
    for v in a:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)


def data(nid, B, off=None):
    """Net and B + 3 input frames of the case (exact_data.net / inputs), targets of the first B and the float64 restatement of one
    bunch, made once and read-only.  off: None = no dropout; else hidden dropout HID_OMIT with the masks of the global frames
    off .. off + B - 1 in step 0 (philox_np.drop_mask; the input layer keeps everything)."""
    if (nid, B, off) not in _DATA:
        c, p = X.exact_case(DC.BY_ID[nid])._replace(B=B), _Bag()
        L = len(c.ls)
        p.c = c
        p.W, p.b = X.net(c)
        p.x = X.inputs(c, B + 3)
        p.mk = None
        if off is not None:
            p.mk = [np.zeros((B, c.ls[0]), np.uint8)] + [P.drop_mask(SEED, 0, l, B, c.ls[l], HID_OMIT, off) for l in range(1, L - 1)]
            for l in range(1, L - 1):
                assert 0.3 < p.mk[l].mean() < 0.7 or B < 8, (nid, B, off, l, p.mk[l].mean())
        rng = np.random.default_rng(1000 * NETS.index(nid) + 10 * B + (0 if off is None else off + 1))
        p.forward = X.Bunch(c, p.W, p.b, p.x, np.zeros((B + 3, c.ls[-1]), np.float32)).out.astype(np.float32)      # inference: no mask
        out = X.Bunch(c, p.W, p.b, p.x[:B], np.zeros((B, c.ls[-1]), np.float32), p.mk).out
        p.d = X.D_VALUES[rng.integers(0, len(X.D_VALUES), size=(B, c.ls[-1]))]
        t = out - p.d * (B / 2.0)
        p.t = t.astype(np.float32)
        assert np.array_equal(p.t.astype(np.float64), t), (nid, B, "the targets are no fp32 numbers")
        p.bunch = bu = X.Bunch(c, p.W, p.b, p.x[:B], p.t, p.mk)
        assert np.array_equal(bu.dx[L - 1], p.d), (nid, B, "dEdX_L is not d")
        for name, A, Bm, add in bu.gemms:
            m, q = X.gemm_bounds(A, Bm, add)
            assert m / q < 2.0 ** 24 and q >= 2.0 ** -40, (nid, B, name, m, q)
        # one fused step from zero momentum, lr 0.5, momentum 0.5, no weight cost: dW = -1/4 G / B, W' = W + dW; exact where B is a
        # power of two (asserted: every value an fp32 number)
        p.step = None
        if B & (B - 1) == 0:
            p.step = [[None], [None], [None], [None]]
            for l in range(1, L):
                for k, (g, w) in enumerate(((bu.gw[l], p.W[l]), (bu.gb[l], p.b[l]))):
                    dw = -0.25 * g / B
                    wn = w.astype(np.float64) + dw
                    assert np.array_equal(dw.astype(np.float32).astype(np.float64), dw) and np.array_equal(wn.astype(np.float32).astype(np.float64), wn), (nid, B, l)
                    p.step[k].append(wn.astype(np.float32))
                    p.step[2 + k].append(dw.astype(np.float32))
        _frozen(p.W[1:] + p.b[1:] + [p.x, p.t, p.forward] + bu.gw[1:] + bu.gb[1:] + ([] if p.step is None else [a for s in p.step for a in s[1:]]))
        _DATA[(nid, B, off)] = p
    return _DATA[(nid, B, off)]


def _mk(pkg, p, B, cap, off=None):
    kw = dict(activation=0, compute_dtype=0, max_chunk_frames=cap)
    if off is not None:
        kw.update(dropoutflag=1, visible_omit=0.0, hid_omit=HID_OMIT, seed=SEED, rank_frame_offset=off)
    return pkg.BP_GPU(1, len(p.c.ls), p.c.ls, B, X.LR, X.MOM, X.WC, p.W, p.b, **kw)


def _step_fails(p, got, what):
    fails, counts = [], {}
    for i, nm in enumerate(("W", "b", "dW", "db")):
        for l in range(1, len(p.c.ls)):
            name = "%s%d" % (nm, l)
            counts[name] = X.count_unequal(got[i][l], p.step[i][l])
            msg = X.unequal(name, got[i][l], p.step[i][l])
            if msg:
                fails.append(msg)
    print(what, "fused step, unequal elements:", counts)
    return fails


def _gradient_fails(p, g, what):
    gw, gb = g.read_grads()
    fails, counts = [], {}
    for l in range(1, len(p.c.ls)):
        for name, a, r in (("G%d" % l, gw[l], p.bunch.gw[l]), ("gb%d" % l, gb[l], p.bunch.gb[l])):
            a = np.asarray(a, np.float32).reshape(np.asarray(r).shape)
            counts[name] = X.count_unequal(a, r)
            msg = X.unequal(name, a, r)
            if msg:
                fails.append(msg)
    print(what, "gradient, unequal elements:", counts)
    return fails


DROP_CASES = [(nid, off) for nid in NETS for off in OFFSETS]


@gpu
@pytest.mark.parametrize("nid,off", DROP_CASES, ids=["%s-off%d" % c for c in DROP_CASES])
def test_dropout_words(pkg, nid, off):
    """One fused step of 64 frames with hid_omit = 0.5 at rank_frame_offset 0 .. 3: every hidden forward draws through one Philox
    block (offset 0) or one of the three straddles of drop_words4, with a key whose halves both have their high bits set (a product
    that lost its upper word, or took it from the wrong multiplicand, would show in half of the units).  The masks reach the weights
    through every layer's output, its dgrad and its weight gradient: all of W, b and the momentum state must be the restatement's."""
    p = data(nid, 64, off)
    g = _mk(pkg, p, 64, 64, off)
    g.train(64, p.x[:64], p.t)
    got = g.get_weights() + g.get_deltas()
    g.close()
    fails = _step_fails(p, got, (nid, off))
    assert not fails, (nid, off, fails)


BLOCK_CASES = [(nid, B) for nid in NETS for B in BUNCHES]


@gpu
@pytest.mark.parametrize("nid,B", BLOCK_CASES, ids=["%s-b%d" % c for c in BLOCK_CASES])
def test_whole_and_partial_blocks(pkg, nid, B):
    """Bunches of 1, 31, 33 and 64 frames: no, one and two 32-row blocks that lie wholly inside the bunch, with and without a partial
    one behind them.  The forward of B + 3 frames (a whole bunch, then three rows of the next), then the stored gradient of one bunch
    with dropout: G_l = y_{l-1}^T dEdX_l sums over the k-tile's rows past the bunch as well, so a dEdX row that a dgrad (or the
    output layer) wrote there, or a missing row inside, shows in the weights' gradient."""
    p = data(nid, B)
    g = _mk(pkg, p, B, B + 3)
    out = g.forward(p.x)
    g.close()
    msg = X.unequal("forward of %d frames" % p.x.shape[0], out, p.forward)
    print(nid, B, "forward, unequal elements:", X.count_unequal(out, p.forward))
    assert msg is None, (nid, B, msg)
    pd = data(nid, B, 0)
    g = _mk(pkg, pd, B, 2 * B, 0)
    g.upload_chunk(pd.x[:B], pd.t)
    g.grads_resident(0)
    fails = _gradient_fails(pd, g, (nid, B))
    g.close()
    assert not fails, (nid, B, fails)


@gpu
@pytest.mark.parametrize("nid", NETS)
def test_partial_bunches_on_one_handle_then_a_step(pkg, nid):
    """One handle of bunch 64: the forward of 64, 33, 31 and 1 frames in turn -- the hidden layers' stores stop at the last frame each
    time, on the same buffers -- and then a fused step of 64 frames.  Every forward and the step are the restatement's bits."""
    p = data(nid, 64)
    g = _mk(pkg, p, 64, 64)
    fails = []
    for n in reversed(BUNCHES):
        out = g.forward(p.x[:n])
        msg = X.unequal("forward of %d frames" % n, out, p.forward[:n])
        if msg:
            fails.append(msg)
    g.train(64, p.x[:64], p.t)
    fails += _step_fails(p, g.get_weights() + g.get_deltas(), nid)
    g.close()
    assert not fails, (nid, fails)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_one_tile_per_workgroup_is_checked_on_the_host(tmp_path):
    """covers_tiles / multi_covers_tiles (csrc/bp_kernels.h), the checks in front of the three launches that wrap GemmKernel::run,
    as a host unit (tests/cpp/one_tile_driver.cc; nothing is launched): a stride shorter than the tile list is refused."""
    exe = str(tmp_path / "one_tile_driver")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "one_tile_driver.cc")])
    out = subprocess.check_output([exe], universal_newlines=True)
    assert "all answered as the contract says" in out, out
