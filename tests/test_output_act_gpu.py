"""GPU tests of the logistic output layer (bp_set_output, -m gpu).  The C oracle only knows the linear output, so the reference
here is float64 torch autograd of the loss (the helpers live in tests/output_ref.py, shared with tests/test_dispatch_gpu.py):
    linear columns [0, lin):     L = (1/Bg) sum (o - t)^2
    logistic columns, loss 0:    L = (2/Bg) sum BCE(y, t)        (dL/dz = (2/Bg)(y - t), BP_GPU.cu.bak:565-630)
    logistic columns, loss 1:    L = (1/Bg) sum (y - t)^2
Dropout masks come from the test's own numpy Philox (tests/philox_np.py).  Bars: fp32 1e-4 relative per tensor, bf16 2e-2 rms."""
import os
import re
import subprocess

import numpy as np
import pytest

import pfile_util as PU
from flip_accounting import relu_flips
from output_ref import _dedz, _trajectory, ref_forward, ref_grads
from philox_np import drop_mask
from util import TOL, relerr

pytestmark = pytest.mark.gpu

SMALL = [40, 96, 72, 33]                     # plain output path (ld_L = 64: one 32x32 / 32x64 launch)
SHIPPED = [129 * 12, 2048, 2048, 2048, 258]  # the reference's geometry, multi-objective: 129 LPS + 129 IBM -> split-K output path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")


def _net(pkg, ls, seed):
    W, b = pkg.glorot_net(ls, seed=seed, beta=0.5)
    rng = np.random.default_rng(seed + 100)
    b = [None] + [(rng.standard_normal(ls[l]) * 0.1).astype(np.float32) for l in range(1, len(ls))]
    return W, b


def _targets(rng, n, sL, lin):
    """[real-valued | binary mask] targets, the multi-objective layout."""
    t = np.empty((n, sL), np.float32)
    t[:, :lin] = rng.standard_normal((n, lin), dtype=np.float32)
    t[:, lin:] = (rng.random((n, sL - lin)) < 0.4).astype(np.float32)
    return t


def _mk(pkg, ls, B, W, b, lr=1.0, m=0.5, **kw):
    return pkg.BP_GPU(1, len(ls), ls, B, lr, m, 0.0, W, b, max_chunk_frames=kw.pop("cap", 4 * B), **kw)


# ------------------------------------------------------------------ 1. gradient of one bunch
@pytest.mark.parametrize("lin,loss", [(0, 0), (16, 0), (16, 1)], ids=["all-logistic-xent", "lin16-xent", "lin16-mse"])
def test_small_net_gradient_matches_float64_autograd(pkg, parity_record, lin, loss):
    pytest.importorskip("torch")
    ls, B = SMALL, 64
    W, b = _net(pkg, ls, 3)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, ls[0]), dtype=np.float32)
    t = _targets(rng, B, ls[-1], lin)
    g = _mk(pkg, ls, B, W, b, activation=1, output_activation=1, output_linear_cols=lin, output_loss=loss)
    g.upload_chunk(x, t)
    g.grads_resident(0)
    gw, gb = g.read_grads()
    g.close()
    tw, tb, _ = ref_grads(ls, W, b, x, t, act=1, lin=lin, loss=loss)
    errs = {}
    for l in range(1, len(ls)):
        errs["W%d" % l], errs["b%d" % l] = relerr(gw[l], tw[l]), relerr(gb[l], tb[l])
    parity_record(config="small %s lin %d loss %d" % (ls, lin, loss), gradient_vs_torch_float64=errs, bar="1e-4")
    assert all(v < TOL for v in errs.values()), errs


def test_shipped_geometry_multi_objective_gradient_on_the_split_path(pkg, parity_record):
    """1548 -> 2048x3 -> 258 (129 linear + 129 logistic), B 128, ReLU, dropout 0.1 / 0.2: the split-K output launch.  ReLU decisions
    within fp32 rounding of zero are counted and their frames removed from both sides (as test_gpu_autograd.py does)."""
    pytest.importorskip("torch")
    ls, B, L, seed, lin = SHIPPED, 128, len(SHIPPED), 23, 129
    W, b = _net(pkg, ls, 1)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((B, ls[0]), dtype=np.float32)
    t = _targets(rng, B, ls[-1], lin)
    g = _mk(pkg, ls, B, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=seed, output_activation=1, output_linear_cols=lin)
    g.upload_chunk(x, t)
    g.grads_resident(0)
    gw, gb = g.read_grads()
    ys_g = [None] + [g.read_layer_output(l) for l in range(1, L - 1)]
    g.close()
    masks = [drop_mask(seed, 0, l, B, ls[l], 0.1 if l == 0 else 0.2) for l in range(L - 1)]
    tw, tb, ys_t = ref_grads(ls, W, b, x, t, masks, lin=lin)
    ys_g[0] = ys_t[0]
    fl = []
    for l in range(1, L - 1):
        assert not ys_g[l][masks[l] == 1].any(), l
        fl += [(l,) + f for f in relu_flips(ys_g[l], ys_t[l], ys_g[l - 1], W[l], b[l])]
    assert len(fl) <= 8, fl
    for l, f, n, mag, scale in fl:
        assert mag <= 64.0 * scale, (l, f, n, mag, scale)
    rows = sorted(set(f for _, f, _, _, _ in fl))
    if rows:
        keep = np.ones(B, bool); keep[rows] = False
        tw, tb, _ = ref_grads(ls, W, b, x, t, masks, lin=lin, keep_rows=keep)
        z = ys_g[L - 2][rows].astype(np.float64) @ W[L - 1].astype(np.float64) + b[L - 1].astype(np.float64)
        dx = {L - 1: _dedz(z, t[rows].astype(np.float64), lin, 0, B)}        # the device's own contribution of those frames
        for l in range(L - 1, 1, -1):
            dx[l - 1] = (ys_g[l - 1][rows] > 0) * (dx[l] @ W[l].astype(np.float64).T)
    errs = {}
    for l in range(1, L):
        Gg, bg = gw[l].astype(np.float64), gb[l].astype(np.float64)
        if rows:
            Gg = Gg - ys_g[l - 1][rows].astype(np.float64).T @ dx[l]
            bg = bg - dx[l].sum(0)
        errs["W%d" % l], errs["b%d" % l] = relerr(Gg, tw[l]), relerr(bg, tb[l])
    parity_record(config="1548-2048x3-258 lin 129 xent B128 dropout", flips=[list(f) for f in fl], gradient_vs_torch_float64=errs, bar="1e-4")
    assert all(v < TOL for v in errs.values()), errs


# ------------------------------------------------------------------ 2. ten-step trajectory
@pytest.mark.parametrize("lin,loss", [(16, 0), (0, 1)], ids=["lin16-xent", "all-logistic-mse"])
def test_small_net_ten_step_trajectory(pkg, parity_record, lin, loss):
    pytest.importorskip("torch")
    ls, B, NS, lr, m = SMALL, 64, 10, 0.5, 0.5
    W, b = _net(pkg, ls, 4)
    rng = np.random.default_rng(12)
    x = rng.standard_normal((NS * B, ls[0]), dtype=np.float32)
    t = _targets(rng, NS * B, ls[-1], lin)
    g = _mk(pkg, ls, B, W, b, lr=lr, m=m, activation=1, cap=NS * B, output_activation=1, output_linear_cols=lin, output_loss=loss)
    g.train(NS * B, x, t)
    w, bb = g.get_weights()
    dw, dbb = g.get_deltas()
    g.close()
    W64, b64, dW64, db64 = _trajectory(ls, W, b, x, t, B, NS, lr, m, 1, lin, loss)
    errs = {}
    for l in range(1, len(ls)):
        errs["W%d" % l], errs["b%d" % l] = relerr(w[l], W64[l]), relerr(bb[l], b64[l])
        errs["dW%d" % l], errs["db%d" % l] = relerr(dw[l], dW64[l]), relerr(dbb[l], db64[l])
    parity_record(config="small lin %d loss %d" % (lin, loss), steps=NS, vs_torch_float64=errs, bar="1e-4")
    assert all(v < TOL for v in errs.values()), errs


def test_shipped_geometry_ten_steps_small_lrate(pkg, parity_record):
    """Multi-objective 1548 -> 2048x3 -> 258, B 128, ReLU, dropout, ten steps at lrate 0.02: outputs of the trained net and every
    weight matrix at the plain 1e-4 bar (momentum state and biases recorded: they carry the ReLU-decision effect)."""
    pytest.importorskip("torch")
    import torch
    ls, B, NS, lr, m, seed, lin = SHIPPED, 128, 10, 0.02, 0.5, 31, 129
    L = len(ls)
    W, b = _net(pkg, ls, 2)
    rng = np.random.default_rng(13)
    x = rng.standard_normal((NS * B, ls[0]), dtype=np.float32)
    t = _targets(rng, NS * B, ls[-1], lin)
    g = _mk(pkg, ls, B, W, b, lr=lr, m=m, cap=NS * B, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=seed,
            output_activation=1, output_linear_cols=lin)
    g.train(NS * B, x, t)
    w, bb = g.get_weights()
    xf = rng.standard_normal((200, ls[0]), dtype=np.float32)
    out_g = g.forward(xf)
    g.close()
    W64, b64, dW64, db64 = _trajectory(ls, W, b, x, t, B, NS, lr, m, 0, lin, 0, drop_seed=seed)
    keep = [None, 0.9] + [0.8] * (L - 2)
    with torch.no_grad():
        _, _, _, _, y = ref_forward(ls, W64, b64, xf, lin=lin, keep=keep)
    errs = {"out": relerr(out_g, y.detach().numpy())}
    for l in range(1, L):
        errs["W%d" % l], errs["b%d" % l] = relerr(w[l], W64[l]), relerr(bb[l], b64[l])
    parity_record(config="1548-2048x3-258 lin 129", lrate=lr, steps=NS, vs_torch_float64=errs, bar="1e-4 on outputs and W; biases recorded")
    assert errs["out"] < TOL, errs
    for l in range(1, L):
        assert errs["W%d" % l] < TOL, (l, errs)


# ------------------------------------------------------------------ 3. CV and forward
@pytest.mark.parametrize("ls,B,lin", [(SMALL, 64, 16), (SHIPPED, 128, 129)], ids=["small", "shipped"])
def test_cv_and_forward_are_post_activation(pkg, parity_record, ls, B, lin):
    pytest.importorskip("torch")
    import torch
    L = len(ls)
    W, b = _net(pkg, ls, 6)
    rng = np.random.default_rng(14)
    n = 3 * B + 17                                                   # partial last bunch
    x = rng.standard_normal((n, ls[0]), dtype=np.float32)
    t = _targets(rng, n, ls[-1], lin)
    g = _mk(pkg, ls, B, W, b, cap=n, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=3, output_activation=1, output_linear_cols=lin)
    cv = g.CrossValid(n, x, t)
    out = g.forward(x)
    g.close()
    keep = [None, 0.9] + [0.8] * (L - 2)
    with torch.no_grad():
        _, _, _, _, y = ref_forward(ls, W, b, x, lin=lin, keep=keep)
    y = y.numpy()
    sq = float(((y - t.astype(np.float64)) ** 2).sum())
    assert out[:, lin:].min() >= 0.0 and out[:, lin:].max() <= 1.0
    assert out[:, :lin].min() < 0.0                                  # the linear columns are not squashed
    errs = {"out": relerr(out, y), "cv_sq_err": abs(cv - sq) / sq}
    parity_record(config="%s lin %d" % (ls, lin), vs_float64=errs, bar="1e-4")
    assert errs["out"] < TOL and errs["cv_sq_err"] < TOL, errs


# ------------------------------------------------------------------ 4. window chunks = stacked chunks
def test_window_chunk_trains_bit_identical_to_stacked(pkg):
    """Logistic output on the split-K launch that also stages the next bunch (visible dropout on): a window chunk and the
    equivalent stacked chunk end with the same weights bit for bit."""
    D, ctx, B, nb, lin = 129, 12, 128, 4, 129
    ls = [D * ctx, 1024, 2 * D]
    W, b = _net(pkg, ls, 7)
    rng = np.random.default_rng(15)
    nf = nb * B + ctx + 40
    fea = rng.standard_normal((nf, D), dtype=np.float32)
    tframes = _targets(rng, nf, ls[-1], lin)
    ws = rng.integers(0, nf - ctx + 1, size=nb * B).astype(np.int32)
    tf = rng.integers(0, nf, size=nb * B).astype(np.int32)
    x = np.stack([fea[s:s + ctx].reshape(-1) for s in ws]).astype(np.float32)
    t = tframes[tf]
    kw = dict(lr=0.5, cap=nb * B, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=8, output_activation=1, output_linear_cols=lin)
    a = _mk(pkg, ls, B, W, b, **kw)
    a.train(nb * B, x, t)
    wa, ba = a.get_weights()
    a.close()
    c = _mk(pkg, ls, B, W, b, **kw)
    c.train_windows(fea, tframes, ctx, ws, tf)
    wc, bc = c.get_weights()
    c.close()
    for l in (1, 2):
        assert np.array_equal(wa[l], wc[l]) and np.array_equal(ba[l], bc[l]), l
    assert not np.array_equal(wa[2], W[2])


# ------------------------------------------------------------------ 5. bf16
def _bf16_ref(ls, W, b, x, t, masks, lin, Bg):
    from torch_ref import bf16_round
    L = len(ls)
    Wb = [None] + [bf16_round(W[l]) for l in range(1, L)]
    h = np.asarray(x, np.float64) * (1.0 - masks[0])
    ys = [bf16_round(h)]
    for l in range(1, L):
        z = ys[l - 1] @ Wb[l] + np.asarray(b[l], np.float64)
        if l < L - 1:
            ys.append(bf16_round(np.maximum(z, 0.0) * (1.0 - masks[l])))
    dx = {L - 1: bf16_round(_dedz(z, np.asarray(t, np.float64), lin, 0, Bg))}
    for l in range(L - 1, 1, -1):
        dx[l - 1] = bf16_round((ys[l - 1] > 0) * (dx[l] @ Wb[l].T))
    return [None] + [ys[l - 1].T @ dx[l] for l in range(1, L)], [None] + [dx[l].sum(0) for l in range(1, L)]


def test_bf16_logistic_gradient_on_the_split_path(pkg, parity_record):
    ls, B, seed, lin = [300, 1024, 1024, 257], 256, 5, 100
    W, b = _net(pkg, ls, 2)
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, ls[0]), dtype=np.float32)
    t = _targets(rng, B, ls[-1], lin)
    g = _mk(pkg, ls, B, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=seed, compute_dtype=1,
            output_activation=1, output_linear_cols=lin)
    g.upload_chunk(x, t)
    g.grads_resident(0)
    gw, gb = g.read_grads()
    g.close()
    masks = [drop_mask(seed, 0, l, B, ls[l], 0.1 if l == 0 else 0.2) for l in range(len(ls) - 1)]
    rw, rb = _bf16_ref(ls, W, b, x, t, masks, lin, B)
    rms = lambda a, r: float(np.sqrt(((np.asarray(a, np.float64) - r) ** 2).sum() / max((r ** 2).sum(), 1e-300)))
    errs = {}
    for l in range(1, len(ls)):
        errs["W%d" % l], errs["b%d" % l] = rms(gw[l], rw[l]), rms(gb[l], rb[l])
    parity_record(config="bf16 %s lin %d" % (ls, lin), gradient_rms_vs_handwritten_bf16_reference=errs, bar="2e-2 rms")
    assert all(v < 2e-2 for v in errs.values()), errs


# ------------------------------------------------------------------ 6. switching back
@pytest.mark.parametrize("ls,B", [(SMALL, 64), (SHIPPED, 128)], ids=["plain", "split"])
def test_switching_back_to_linear_is_bit_identical(pkg, ls, B):
    """After logistic steps, bp_set_output(0, 0, 0) makes the next steps those of a handle that was linear throughout, from the
    same weights (momentum 0: the momentum state does not enter the next step)."""
    W, b = _net(pkg, ls, 9)
    rng = np.random.default_rng(16)
    x = rng.standard_normal((4 * B, ls[0]), dtype=np.float32)
    t = _targets(rng, 4 * B, ls[-1], ls[-1] // 2)
    a = _mk(pkg, ls, B, W, b, lr=0.3, m=0.0, cap=4 * B, output_activation=1, output_linear_cols=ls[-1] // 2, output_loss=1)
    a.train(2 * B, x[:2 * B], t[:2 * B])
    w_mid, b_mid = a.get_weights()
    assert not np.array_equal(w_mid[len(ls) - 1], W[len(ls) - 1])
    a.set_output(0)
    a.train(2 * B, x[2 * B:], t[2 * B:])
    wa, ba = a.get_weights()
    da, dba = a.get_deltas()
    a.close()
    c = _mk(pkg, ls, B, w_mid, b_mid, lr=0.3, m=0.0, cap=4 * B)
    c.train(2 * B, x[2 * B:], t[2 * B:])
    wc, bc = c.get_weights()
    dc, dbc = c.get_deltas()
    c.close()
    for l in range(1, len(ls)):
        assert np.array_equal(wa[l], wc[l]) and np.array_equal(ba[l], bc[l]), l
        assert np.array_equal(da[l], dc[l]) and np.array_equal(dba[l], dbc[l]), l


# ------------------------------------------------------------------ 7. data parallel
def test_data_parallel_two_ranks_match_one_handle(pkg, parity_record):
    """2 ranks on one device, native transport, multi-objective output, sigmoid hidden layers: the weights equal one handle with
    the global bunch at 1e-4."""
    import json
    import subprocess as sp
    import sys
    import tempfile
    from output_act_dp_worker import case_data, shard_rows
    world, B, nb = 2, 64, 4
    c = dict(ls=[300, 512, 256, 130], B=B, world=world, nb=nb, lin=65, key="oa%d" % os.getpid())
    W, b, x, t = case_data(c)
    with tempfile.TemporaryDirectory() as td:
        cj = os.path.join(td, "case.json")
        json.dump(c, open(cj, "w"))
        env = dict(os.environ, BP_DP_TIMEOUT_S="60", HSA_ENABLE_IPC_MODE_LEGACY="0")
        here = os.path.dirname(os.path.abspath(__file__))
        procs = [sp.Popen([sys.executable, os.path.join(here, "output_act_dp_worker.py"), cj, str(r), td], env=env,
                          stdout=sp.PIPE, stderr=sp.STDOUT) for r in range(world)]
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=300)[0].decode(errors="replace"))
            except sp.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
        for r, p in enumerate(procs):
            assert p.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])
        res = [dict(np.load(os.path.join(td, "rank%d.npz" % r))) for r in range(world)]
    ls = c["ls"]
    g = pkg.BP_GPU(1, len(ls), ls, B * world, 0.5, 0.5, 0.0, W, b, activation=1, max_chunk_frames=nb * B * world,
                   output_activation=1, output_linear_cols=c["lin"])
    g.train(x.shape[0], x, t)
    w1, b1 = g.get_weights()
    g.close()
    errs = {}
    for l in range(1, len(ls)):
        for r in range(world):
            errs["W%d_r%d" % (l, r)] = relerr(res[r]["W%d" % l], w1[l])
            errs["b%d_r%d" % (l, r)] = relerr(res[r]["b%d" % l], b1[l])
    parity_record(config="dp 2 ranks %s lin %d" % (ls, c["lin"]), vs_single_handle=errs, bar="1e-4")
    assert all(v < TOL for v in errs.values()), errs
    assert not np.array_equal(w1[len(ls) - 1], W[len(ls) - 1])


# ------------------------------------------------------------------ 8. command line
def _exe(name):
    exe = os.path.join(PKG, name)
    if not os.path.exists(exe):
        import __graft_entry__
        __graft_entry__.build()
    return exe


def test_bptrain_and_bpforward_multi_objective_match_the_python_mirror(pkg, tmp_path):
    """bptrain on a 129-bin Pfile pair with [LPS | IBM] targets, output_act=sigmoid output_linear_dims=129: its .wts equal the Python
    mirror driving the same chunks bit for bit, its CV line equals the mirror's CrossValid; bpforward with the same keys equals
    bp_forward bit for bit."""
    D, ctx, toff, seed, cache, B = 129, 3, 1, 345, 64, 16
    ls = [D * (ctx + 1), 96, 2 * D]                                   # NAT block appended
    lens = [30, 22, 41, 8, 27, 35, 19, 26, 33, 24]
    rs = np.random.default_rng(19)
    n = sum(lens)
    fea = rs.normal(size=(n, D)).astype(np.float32)
    tg = _targets(rs, n, 2 * D, D)
    mean, istd = np.zeros(D, np.float32), np.ones(D, np.float32)    # identity normalisation: the rows the mirror sees are exact
    p = {k: str(tmp_path / v) for k, v in dict(fea="f.pfile", targ="t.pfile", norm="n.norm", init="mlp.0.wts",
                                               out="mlp.1.wts", log="mlp.1.log", enh="enh.pfile").items()}
    PU.write_pfile(p["fea"], lens, fea); PU.write_pfile(p["targ"], lens, tg); PU.write_norm(p["norm"], mean, istd)
    W = [None] + [(rs.normal(size=(ls[l - 1], ls[l])) * 0.1).astype(np.float32) for l in (1, 2)]
    b = [None] + [(rs.normal(size=ls[l]) * 0.1).astype(np.float32) for l in (1, 2)]
    PU.write_wts(p["init"], ls, W, b)
    keys = ["output_act=sigmoid", "output_linear_dims=%d" % D]
    args = ["fea_file=" + p["fea"], "targ_file=" + p["targ"], "norm_file=" + p["norm"], "initwts_file=" + p["init"],
            "outwts_file=" + p["out"], "log_file=" + p["log"], "train_sent_range=0-7", "cv_sent_range=8-9",
            "fea_dim=%d" % D, "fea_context=%d" % ctx, "targ_offset=%d" % toff, "dropoutflag=0", "traincache=%d" % cache,
            "bunchsize=%d" % B, "gpu_used=1", "init_randem_seed=%d" % seed, "momentum=0.5", "weightcost=0.0", "lrate=0.5",
            "visible_omit=0.0", "hid_omit=0.0", "layersizes=%s" % ",".join(map(str, ls)), "stack=host"] + keys
    r = subprocess.run([_exe("bptrain")] + args, capture_output=True, text=True)
    assert r.returncode == 1, r.stdout + r.stderr
    bad = subprocess.run([_exe("bptrain")] + args[:-2] + ["output_act=softmax"], capture_output=True, text=True)
    assert bad.returncode == 0 and "output_act" in bad.stdout            # strict key: message + exit(0)
    fb = np.cumsum(lens).tolist(); sent_of = np.repeat(np.arange(len(lens)), lens)
    r48 = PU.Rand48(seed)
    starts, total = PU.plan(fb, n, ctx, cache, 0, 7)
    order_chunks = PU.rand_index(len(starts), r48)
    g = pkg.BP_GPU(1, 3, ls, B, 0.5, 0.5, 0.0, W, b, max_chunk_frames=cache, output_activation=1, output_linear_cols=D)
    for ci in order_chunks:
        cnt = total - cache * ci if ci == len(starts) - 1 else cache
        xin, xtg = PU.read_chunk(fea, tg, sent_of, fb, mean, istd, starts, total, 7, ci, ctx, cache, toff, True, PU.rand_index(cnt, r48))
        g.train(cnt, xin, xtg)
    Wm, bm = g.get_weights()
    Wg, bg = PU.read_wts(p["out"], ls)
    for l in (1, 2):
        assert np.array_equal(Wg[l], Wm[l]) and np.array_equal(bg[l], bm[l]), l
    cstarts, ctotal = PU.plan(fb, n, ctx, cache, 8, 9)
    sq = np.float32(0.0)
    for ci in range(len(cstarts)):
        cnt = ctotal - cache * ci if ci == len(cstarts) - 1 else cache
        xin, xtg = PU.read_chunk(fea, tg, sent_of, fb, mean, istd, cstarts, ctotal, 9, ci, ctx, cache, toff, True, list(range(cnt)))
        sq = np.float32(sq + np.float32(g.CrossValid(cnt, xin, xtg)))
    m = re.search(r"CV over\. squared error: (\S+)", open(p["log"]).read())
    assert m and m.group(1) == "%f" % np.float32(sq / np.float32(ctotal)), (m.group(1) if m else None, sq / ctotal)
    # bpforward with the same keys: every window of sentences 8-9, against bp_forward on the same rows
    fargs = ["fea_file=" + p["fea"], "norm_file=" + p["norm"], "initwts_file=" + p["out"], "out_file=" + p["enh"],
             "layersizes=%s" % ",".join(map(str, ls)), "fea_dim=%d" % D, "fea_context=%d" % ctx, "targ_offset=%d" % toff,
             "sent_range=8-9", "bunchsize=%d" % B] + keys
    r = subprocess.run([_exe("bpforward")] + fargs, capture_output=True, text=True)
    assert r.returncode == 1, r.stdout + r.stderr
    rows = PU.expected_windows(fea, lens, mean, istd, ctx, True)    # every window of every sentence, file order
    first = sum(max(0, ln - ctx + 1) for ln in lens[:8])
    want = g.forward(rows[first:])
    g.close()
    got = _read_pfile_features(p["enh"], 2 * D)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert got[:, D:].min() >= 0.0 and got[:, D:].max() <= 1.0


def _read_pfile_features(path, dim):
    raw = open(path, "rb").read()
    hdr = raw[:32768].decode(errors="replace")
    nfr = int(re.search(r"-num_frames (\d+)", hdr).group(1))
    rec = np.frombuffer(raw[32768:32768 + nfr * (2 + dim) * 4], ">u4").reshape(nfr, 2 + dim)
    return rec[:, 2:].astype(np.uint32).view(np.float32)
