"""Pre-training on the GPU (the bp_rbm_* block of include/bp_c_api.h, csrc/bp_rbm.hip): every stage of a CD-1 step held to float64
on the device's own operands, the update held to float64 from the device's stored gradients, ten mean-field steps against the
float64 restatement of the same steps, determinism and keying, the stack, learning, the hand-over to a sigmoid BP_GPU handle and
the bppretrain tool.  Data, stacks, hyper sets, bars and the checks are those of tests/rbm_np.py; tests/test_rbm_host.py shows on
the CPU which wrong implementations the checks would see."""
import os
import re
import subprocess

import numpy as np
import pytest

import pfile_util as PU
import rbm_np as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")
LAYERS = [(sid, l) for sid, st in R.STACKS.items() for l in range(1, len(st.sizes))]
LAYER_IDS = ["%s-l%d" % p for p in LAYERS]
_ROWS = {}


def rows(sid):
    """The stack's rows, computed once and never written to."""
    if sid not in _ROWS:
        _ROWS[sid] = R.rows(R.STACKS[sid])
        _ROWS[sid].setflags(write=False)
    return _ROWS[sid]


def open_stack(pkg, sid, seed=R.SEED, cap=None):
    st = R.STACKS[sid]
    W, c, a = R.params(st)
    s = pkg.rbm_open(0, st.sizes, st.bunch, W, c, a, seed=seed, max_chunk_frames=cap or R.N_BUNCHES * st.bunch)
    return s, st, (W, c, a)


def same(x, y):
    return all(np.array_equal(p, q) for xs, ys in zip(x, y) for p, q in zip(xs[1:], ys[1:]))


# ------------------------------------------------------------------ 1. the stages of one step
@pytest.mark.parametrize("sample", [1, 0], ids=["sampled", "meanfield"])
@pytest.mark.parametrize("sid,layer", LAYERS, ids=LAYER_IDS)
def test_every_stage_of_a_step_against_float64_on_the_devices_own_operands(pkg, parity_record, sid, layer, sample):
    s, st, (W, c, a) = open_stack(pkg, sid)
    B, V, H = st.bunch, st.sizes[layer - 1], st.sizes[layer]
    visible = 0 if layer == 1 else 1
    assert s.hyper(layer)["visible"] == visible
    s.set_hyper(layer, sample=sample)
    before, n_before = s.get(), [s.steps(l) for l in range(1, len(st.sizes))]
    tr = s.step(layer, rows(sid)[:B])
    assert [tr[k].shape for k in ("v0", "p0", "s0", "v1", "p1", "gw", "gc", "ga")] == [(B, V), (B, H), (B, H), (B, V), (B, H), (V, H), (H,), (V,)]
    assert all(np.isfinite(tr[k]).all() for k in tr)
    if layer == 1:
        assert np.array_equal(tr["v0"], rows(sid)[:B])
    e = R.stage_errors(tr, W[layer], c[layer], a[layer], visible, sample, R.uniforms(R.SEED, 0, layer, B, H))
    print(sid, layer, sample, " ".join("%s %.3g" % kv for kv in sorted(e.items())))
    parity_record(**{"bars_" + k: v for k, v in e.items()})
    assert all(v <= 1.0 for v in e.values()), e
    if sample:
        assert set(np.unique(tr["s0"])) <= {0.0, 1.0} and 0.1 < tr["s0"].mean() < 0.9
    else:
        assert np.array_equal(tr["s0"], tr["p0"])
    # apply = 0: nothing of the stack has changed
    assert same(s.get(), before) and [s.steps(l) for l in range(1, len(st.sizes))] == n_before == [0] * (len(st.sizes) - 1)
    s.close()


# ------------------------------------------------------------------ 2. the update
@pytest.mark.parametrize("hset", ["A", "B"])
@pytest.mark.parametrize("sid,layer", LAYERS, ids=LAYER_IDS)
def test_two_applied_steps_against_float64_from_the_stored_gradients(pkg, parity_record, sid, layer, hset):
    s, st, _ = open_stack(pkg, sid)
    B, H, hy = st.bunch, st.sizes[layer], R.HYPER[hset]
    visible = 0 if layer == 1 else 1
    s.set_hyper(layer, lrate=hy.lrate, momentum=hy.momentum, weightcost=hy.weightcost, sample=1)
    pick = lambda g: (g[0][layer], g[1][layer], g[2][layer])
    state = tuple(np.zeros_like(x, dtype=np.float64) for x in pick(s.get()))
    worst = {}
    for i in range(2):
        x = rows(sid)[i * B:(i + 1) * B]
        old = pick(s.get())
        tr = s.step(layer, x)                               # the stored gradients, at the counter the applied step will use
        ap = s.step(layer, x, apply=True)
        assert all(np.array_equal(tr[k], ap[k]) for k in ("p0", "s0", "v1", "p1", "gw", "gc", "ga")) and tr["recon"] == ap["recon"]
        e, state = R.update_errors(hy, B, old, state, (tr["gw"], tr["gc"], tr["ga"]), pick(s.get()))
        print(sid, layer, hset, i, e)
        worst.update({"%s_step%d" % (k, i): v for k, v in e.items()})
        assert all(v <= 1.0 for v in e.values()), (i, e)
        assert s.steps(layer) == i + 1
    # ... and a step on the moved weights passes the stage checks (what leaves the pad columns of W non-zero shows here)
    Wn, cn, an = pick(s.get())
    tr = s.step(layer, rows(sid)[2 * B:3 * B])
    e = R.stage_errors(tr, Wn, cn, an, visible, 1, R.uniforms(R.SEED, 2, layer, B, H))
    parity_record(stage_bars_after=e, **worst)
    assert all(v <= 1.0 for v in e.values()), e
    s.close()


# ------------------------------------------------------------------ 3. ten steps
@pytest.mark.parametrize("sid,layer", [p for p in LAYERS if p[0] in ("S", "W")], ids=[i for p, i in zip(LAYERS, LAYER_IDS) if p[0] in ("S", "W")])
def test_ten_meanfield_steps_against_the_float64_restatement(pkg, parity_record, sid, layer):
    s, st, (W, c, a) = open_stack(pkg, sid)
    B, hy = st.bunch, R.Hyper(0.002, 0.9, 1e-5)
    s.set_hyper(layer, lrate=hy.lrate, momentum=hy.momentum, weightcost=hy.weightcost, sample=0)
    x = rows(sid)[:10 * B]
    v = x if layer == 1 else s.up(layer - 1, x)             # (the layers below do not move: their outputs are the restatement's data)
    (Wr, cr, ar), rec = R.meanfield_steps(v, B, W[layer], c[layer], a[layer], 0 if layer == 1 else 1, hy, 10)
    recon = s.train(layer, x)
    g = s.get()
    e = {"W": R.relmax(g[0][layer], Wr), "c": R.relmax(g[1][layer], cr), "a": R.relmax(g[2][layer], ar), "recon": abs(recon - sum(rec)) / sum(rec)}
    print(sid, layer, e)
    parity_record(**e)
    assert all(v <= R.TEN_STEP_BAR for v in e.values()), e
    assert s.steps(layer) == 10
    s.close()


# ------------------------------------------------------------------ 4. determinism and keying
def test_two_stacks_given_the_same_calls_hold_the_same_bits(pkg):
    sid = "W"
    B = R.STACKS[sid].bunch
    x = rows(sid)
    s1, st, _ = open_stack(pkg, sid)
    s2, _, _ = open_stack(pkg, sid)
    r1 = [s1.train(1, x), s1.train(2, x)]
    r2 = [s2.train(1, x[:5 * B]) + s2.train(1, x[5 * B:]), s2.train(2, x)]
    assert same(s1.get(), s2.get()) and r1[1] == r2[1] and abs(r1[0] - r2[0]) <= 1e-12 * r1[0]
    assert s1.steps(1) == s1.steps(2) == R.N_BUNCHES
    # train == the same bunches through step(apply=True)
    s3, _, _ = open_stack(pkg, sid)
    rec = [s3.step(1, x[i * B:(i + 1) * B], apply=True)["recon"] for i in range(R.N_BUNCHES)]
    s4, _, _ = open_stack(pkg, sid)
    assert s4.train(1, x) == sum(rec[1:], rec[0]) and same(s3.get(), s4.get())
    for s in (s1, s2, s3, s4):
        s.close()


def test_seed_counter_and_the_partial_last_bunch(pkg):
    sid = "S"
    st = R.STACKS[sid]
    B, x = st.bunch, rows(sid)
    s, _, _ = open_stack(pkg, sid)
    t, _, _ = open_stack(pkg, sid, seed=R.SEED + 1)
    a0, b0 = s.step(1, x[:B]), t.step(1, x[:B])
    assert np.array_equal(a0["p0"], b0["p0"]) and not np.array_equal(a0["s0"], b0["s0"])
    before = s.get()
    assert s.train(1, x[:B - 1]) == 0.0 and same(s.get(), before) and s.steps(1) == 0          # short of one bunch: nothing
    assert s.train(1, x[:2 * B + 5]) > 0.0 and s.steps(1) == 2 and s.steps(2) == 0
    u, _, _ = open_stack(pkg, sid)
    u.train(1, x[:2 * B])
    assert same(s.get(), u.get())                                                               # the 5 rows behind changed nothing
    s.step(1, x[:B])
    assert s.steps(1) == 2                                                                      # applied bunches only
    a2 = s.step(1, x[:B])
    assert not np.array_equal(a2["s0"], a0["s0"])                                               # the counter keys the samples
    with pytest.raises(pkg.BPError):
        s.train(1, np.zeros((R.N_BUNCHES * B + 1, st.sizes[0]), np.float32))                    # over the capacity
    with pytest.raises(pkg.BPError):
        s.train(3, x[:B])
    assert same(s.get(), u.get()) and s.steps(1) == 2
    for q in (s, t, u):
        q.close()


# ------------------------------------------------------------------ 5. the stack
def test_the_layers_below_feed_a_layer_their_mean_field_and_stay_as_they_are(pkg, parity_record):
    sid = "S"
    st = R.STACKS[sid]
    B, x = st.bunch, rows(sid)
    s, _, (W, c, a) = open_stack(pkg, sid)
    assert np.array_equal(s.step(2, x[:B])["v0"], s.up(1, x[:B]))
    before = s.get()
    s.train(2, x[:4 * B])
    after = s.get()
    assert all(np.array_equal(before[k][1], after[k][1]) for k in range(3)) and not np.array_equal(before[0][2], after[0][2])
    worst = 0.0
    for n in (1, 23, 24, 25, 100):
        h1 = R.sig(x[:n].astype(np.float64) @ W[1] + c[1])
        y1, y2 = s.up(1, x[:n]), s.up(2, x[:n])
        assert y1.shape == (n, st.sizes[1]) and y2.shape == (n, st.sizes[2])
        e1 = R.relmax(y1, h1)
        e2 = R.relmax(y2, R.sig(y1.astype(np.float64) @ after[0][2] + after[1][2]))
        worst = max(worst, e1, e2)
        assert e1 <= R.GEMM_BAR and e2 <= R.GEMM_BAR, (n, e1, e2)
    parity_record(up_worst=worst)
    s.close()


# ------------------------------------------------------------------ 6. learning
@pytest.mark.parametrize("layer", [1, 2])
def test_the_reconstruction_error_falls_every_epoch(pkg, parity_record, layer):
    s, st, _ = open_stack(pkg, "W")
    x = rows("W")
    hy = (0.002, 0.5, 1e-4) if layer == 1 else (0.05, 0.5, 1e-4)
    s.set_hyper(layer, lrate=hy[0], momentum=hy[1], weightcost=hy[2], sample=1)
    rec = [s.train(layer, x) for _ in range(5)]
    print(layer, rec)
    parity_record(recon_per_epoch=rec)
    assert all(b < a for a, b in zip(rec, rec[1:])), rec
    s.close()


# ------------------------------------------------------------------ 7. the hand-over to the net
def test_a_sigmoid_net_made_from_the_stack_computes_the_stacks_hidden_layer(pkg, parity_record):
    sid = "S"
    st = R.STACKS[sid]
    B, x = st.bunch, rows(sid)
    s, _, _ = open_stack(pkg, sid)
    s.train(1, x[:3 * B])
    W, c, _ = s.get()
    ls = list(st.sizes) + [17]
    rng = np.random.default_rng(3)
    Wn = W + [(0.1 * rng.standard_normal((ls[-2], ls[-1]))).astype(np.float32)]
    bn = c + [np.zeros(ls[-1], np.float32)]
    g = pkg.BP_GPU(1, len(ls), ls, B, 0.1, 0.5, 0.0, Wn, bn, activation=1, max_chunk_frames=4 * B)
    g.upload_chunk(x[:B], np.zeros((B, ls[-1]), np.float32))
    g.grads_resident(0)
    e1 = R.relmax(g.read_layer_output(1), s.up(1, x[:B]))
    e2 = R.relmax(g.read_layer_output(2), s.up(2, x[:B]))
    parity_record(hidden1=e1, hidden2=e2)
    assert e1 <= R.GEMM_BAR and e2 <= R.GEMM_BAR, (e1, e2)
    g.close()
    s.close()


# ------------------------------------------------------------------ 8. the tool
def test_bppretrain_writes_a_net_that_bptrain_starts_from(tmp_path):
    D, ctx, B, cache = 33, 7, 32, 200
    ls = [D * ctx, 96, 64, D]
    lens = [60, 45, 80, 52, 71, 66]
    rng = np.random.default_rng(5)
    n = sum(lens)
    z = (rng.random((n, 8)) < 0.5).astype(np.float64)
    fea = (z @ rng.standard_normal((8, D)) + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    tg = rng.standard_normal((n, D)).astype(np.float32)
    p = lambda name: str(tmp_path / name)
    PU.write_pfile(p("f.pfile"), lens, fea)
    PU.write_pfile(p("t.pfile"), lens, tg)
    PU.write_norm(p("norm"), fea.mean(0).astype(np.float32), (1.0 / fea.std(0)).astype(np.float32))
    W = [None] + [(0.1 * rng.standard_normal((ls[l - 1], ls[l]))).astype(np.float32) for l in (1, 2, 3)]
    b = [None] + [(0.1 * rng.standard_normal(ls[l])).astype(np.float32) for l in (1, 2, 3)]
    PU.write_wts(p("init.wts"), ls, W, b)
    for exe in ("bppretrain", "bptrain"):
        assert os.path.exists(os.path.join(PKG, exe)), exe
    common = ["fea_file=" + p("f.pfile"), "norm_file=" + p("norm"), "fea_dim=%d" % D, "fea_context=%d" % ctx, "targ_offset=3",
              "numlayers=4", "layersizes=" + ",".join(map(str, ls)), "bunchsize=%d" % B, "traincache=%d" % cache, "init_randem_seed=11"]
    outs = []
    for run in (1, 2):
        args = common + ["train_sent_range=0-5", "initwts_file=" + p("init.wts"), "outwts_file=" + p("pre%d.wts" % run), "log_file=" + p("pre%d.log" % run),
                         "rbm_epochs=2", "rbm_lrate=0.002,0.05", "rbm_momentum=0.5", "seed=9"]
        r = subprocess.run([os.path.join(PKG, "bppretrain")] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all finish!" in r.stdout, r.stdout + r.stderr
        outs.append(open(p("pre%d.wts" % run), "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 4 * ls[0] * ls[1]
    Wp, bp_ = PU.read_wts(p("pre1.wts"), ls)
    assert np.array_equal(Wp[3], W[3]) and np.array_equal(bp_[3], b[3])
    init = open(p("init.wts"), "rb").read()
    at = init.find(W[3].tobytes()[:256]) - 30                           # the output layer from its matrix header on (20 bytes + "weights34\0")
    assert at > 0 and init[at + 20:at + 29] == b"weights34" and len(init) == len(outs[0])
    assert outs[0][at:] == init[at:] and outs[0][:at] != init[:at]
    for l in (1, 2):
        assert not np.array_equal(Wp[l], W[l]) and not np.array_equal(bp_[l], b[l])
    log = open(p("pre1.log")).read()
    for l in (1, 2):
        e = [float(m) for m in re.findall(r"RBM layer %d epoch \d+: reconstruction error per frame (\S+)" % l, log)]
        assert len(e) == 2 and e[1] < e[0], (l, e)
    args = common + ["targ_file=" + p("t.pfile"), "train_sent_range=0-3", "cv_sent_range=4-5", "initwts_file=" + p("pre1.wts"), "outwts_file=" + p("ft.wts"),
                     "log_file=" + p("ft.log"), "activation=sigmoid", "dropoutflag=0", "gpu_used=1", "momentum=0.5", "weightcost=0", "lrate=0.1"]
    r = subprocess.run([os.path.join(PKG, "bptrain")] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "all finish!" in r.stdout, r.stdout + r.stderr
    ft = open(p("ft.log")).read()
    assert "Init weight file loaded." in ft and "Starting chunk 1 of" in ft and "CV over. squared error:" in ft
    Wf, _ = PU.read_wts(p("ft.wts"), ls)
    assert np.isfinite(Wf[1]).all() and not np.array_equal(Wf[1], Wp[1])
