"""GPU tests of the signal layer (bp_enhance_waves, bp_wave_lps; -m gpu) against the float64 NumPy restatement in
tests/wave_np.py.  Bars: analysis and resynthesis 1e-5 of the largest magnitude, the net outputs 1e-4 (fp32) / 2e-2 (bf16)
relative (util.relerr)."""
import numpy as np
import pytest

import wave_np as WN
from util import TOL, relerr

pytestmark = pytest.mark.gpu

D = 129           # the shipped geometry: n_fft 256, hop 128


def _handle(pkg, ls, W, b, B=64, cap=20000, **kw):
    return pkg.BP_GPU(1, len(ls), ls, B, 0.0, 0.0, 0.0, W, b, max_chunk_frames=cap, **kw)


def _stats(xs, fea_dim):
    m, i = WN.norm_stats(xs, fea_dim)
    return m.astype(np.float32), i.astype(np.float32)


def _wave_err(got, xs):
    return max(float(np.abs(np.asarray(g, np.float64) - x).max()) / float(np.abs(x).max()) for g, x in zip(got, xs))


# ---- 1. analysis
@pytest.mark.parametrize("fea_dim", [33, 65, 129, 257, 513, 1025])
def test_analysis_matches_numpy(pkg, fea_dim, parity_record):
    n_fft, hop = WN.geometry(fea_dim)
    rng = np.random.default_rng(fea_dim)
    lens = [1, hop - 1, n_fft - 1] + [int(v) for v in rng.integers(1, 6 * n_fft, size=4)] + [3 * hop]
    xs = WN.make_sentences(rng, lens)
    xs[-1][:] = 0.0                                   # a silent sentence: every bin at the floor
    got = pkg.wave_lps(0, fea_dim, xs)
    worst, floors = 0.0, 0
    for x, l in zip(xs, got):
        Y = WN.analysis(x, fea_dim)
        assert l.shape == Y.shape
        mag = np.abs(Y)
        below = mag ** 2 < 1e-10
        assert np.all(l[below] == np.float32(WN.LN_FLOOR)), "bins below the floor must be exactly ln(1e-10)"
        floors += int(below.sum())
        for t in range(Y.shape[0]):
            if mag[t].max() > 0:
                e = np.abs(np.exp(l[t].astype(np.float64) / 2) - mag[t]).max() / mag[t].max()
                worst = max(worst, e)
    parity_record(max_rel_mag_err=worst, floor_bins=floors)
    assert floors > 0
    assert worst <= 1e-5, worst


# ---- 2. identity round trip
@pytest.mark.parametrize("ctx,toff", [(1, 0), (7, 0), (7, 3), (7, 6)])
@pytest.mark.parametrize("nat", [False, True])
def test_identity_round_trip(pkg, ctx, toff, nat, parity_record):
    rng = np.random.default_rng(100 * ctx + toff + (7 if nat else 0))
    xs = WN.make_sentences(rng, [1, 127, 255, 1000, 4321, 777])
    m, i = _stats(xs, D)
    ls, W, b = WN.identity_net(D, ctx, toff, nat, m, i)
    g = _handle(pkg, ls, W, b, B=16)                 # 59 frames: three bunches and a partial one
    try:
        got, net = g.enhance_waves(xs, m, i, ctx, toff, return_net=True)
    finally:
        g.close()
    assert [a.size for a in got] == [x.size for x in xs]
    assert sum(n.shape[0] for n in net) % 16 != 0
    err = _wave_err(got, xs)
    parity_record(max_rel_wave_err=err)
    assert err <= 1e-5, err


# ---- 3. mask mode
def test_mask_identity_and_random_mask(pkg, parity_record):
    rng = np.random.default_rng(3)
    xs = WN.make_sentences(rng, [500, 2000, 129])
    m, i = _stats(xs, D)
    ls = [3 * D, 64, D]
    W = [None, np.zeros((3 * D, 64), np.float32), np.zeros((64, D), np.float32)]
    b = [None, np.zeros(64, np.float32), np.full(D, 40.0, np.float32)]
    g = _handle(pkg, ls, W, b, output_activation=1)
    try:
        got = g.enhance_waves(xs, m, i, 3, 1, target=pkg.WAVE_MASK)
        e_id = _wave_err(got, xs)
        g.close()
        W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
        g = _handle(pkg, ls, W, b, output_activation=1)
        got, net = g.enhance_waves(xs, m, i, 3, 1, target=pkg.WAVE_MASK, return_net=True)
    finally:
        g.close()
    e_rand = 0.0
    for x, y, o in zip(xs, got, net):
        assert 0.0 < o.min() and o.max() < 1.0
        ref = WN.resynth(WN.analysis(x, D), o, 1, x.size)
        e_rand = max(e_rand, float(np.abs(y - ref).max() / np.abs(ref).max()))
    parity_record(identity_mask_err=e_id, random_mask_err=e_rand)
    assert e_id <= 1e-5, e_id
    assert e_rand <= 1e-5, e_rand


# ---- 4. random ReLU net with NAT and dropout keep-scaling; 6. the same in bf16
def _random_net_case(pkg, compute_dtype):
    rng = np.random.default_rng(4)
    xs = WN.make_sentences(rng, [3000, 1, 900, 6000])
    m, i = _stats(xs, D)
    ctx, toff = 5, 2
    ls = [(ctx + 1) * D, 256, 256, D]
    W, b = pkg.glorot_net(ls, seed=9, beta=0.5)
    g = _handle(pkg, ls, W, b, B=32, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, compute_dtype=compute_dtype)
    try:
        got, net = g.enhance_waves(xs, m, i, ctx, toff, return_net=True)
    finally:
        g.close()
    e_net = e_wave = 0.0
    for x, y, o in zip(xs, got, net):
        Y = WN.analysis(x, D)
        z = (WN.lps(Y) - m) * i
        ref = WN.forward(W, b, WN.stack(z, ctx, toff, True), keep=(0.9, 0.8))
        e_net = max(e_net, relerr(o, ref))
        r = WN.resynth(Y, o, 0, x.size)
        e_wave = max(e_wave, float(np.abs(y - r).max() / np.abs(r).max()))
    return e_net, e_wave


def test_random_net_nat_dropout(pkg, parity_record):
    e_net, e_wave = _random_net_case(pkg, 0)
    parity_record(out_net_relerr=e_net, wave_err=e_wave)
    assert e_net <= TOL, e_net
    assert e_wave <= 1e-5, e_wave


def test_bf16_handle(pkg, parity_record):
    e_net, e_wave = _random_net_case(pkg, 1)
    parity_record(out_net_relerr=e_net, wave_err=e_wave)
    assert e_net <= 2e-2, e_net
    assert e_wave <= 1e-5, e_wave


# ---- 5. multi-objective net: columns [0, D) LPS (identity minus 6 dB), [D, 2D) logistic mask (= 1)
def test_multi_objective_columns(pkg, parity_record):
    rng = np.random.default_rng(5)
    xs = WN.make_sentences(rng, [1500, 400])
    m, i = _stats(xs, D)
    ls, W, b = WN.identity_net(D, 3, 1, False, m, i)
    ls[-1] = 2 * D
    W[2] = np.concatenate([W[2], np.zeros_like(W[2])], axis=1)
    b[2] = np.concatenate([b[2] + np.float32(2 * np.log(0.5)), np.full(D, 40.0, np.float32)]).astype(np.float32)
    g = _handle(pkg, ls, W, b, output_activation=1, output_linear_cols=D)
    try:
        half = g.enhance_waves(xs, m, i, 3, 1, target=pkg.WAVE_LPS, out_col=0)
        full, net = g.enhance_waves(xs, m, i, 3, 1, target=pkg.WAVE_MASK, out_col=D, return_net=True)
    finally:
        g.close()
    assert net[0].shape[1] == 2 * D
    e_half = _wave_err([2 * h for h in half], xs)
    e_full = _wave_err(full, xs)
    parity_record(lps_cols_err=e_half, mask_cols_err=e_full)
    assert e_half <= 1e-5 and e_full <= 1e-5, (e_half, e_full)


# ---- 7. determinism
def test_bit_identical_runs(pkg):
    rng = np.random.default_rng(7)
    xs = WN.make_sentences(rng, [5000, 333, 2])
    m, i = _stats(xs, D)
    ls = [(7 + 1) * D, 256, D]
    W, b = pkg.glorot_net(ls, seed=2, beta=0.5)
    g = _handle(pkg, ls, W, b)
    try:
        a = g.enhance_waves(xs, m, i, 7, 3)
        c = g.enhance_waves(xs, m, i, 7, 3)
    finally:
        g.close()
    for u, v in zip(a, c):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


# ---- 8. training is not disturbed by an enhancement call in between
FD = 33                                                  # n_fft 64


def _train_pair(pkg, windows, enhance):
    ctx, B = 3, 32
    ls = [ctx * FD, 64, FD]
    W, b = pkg.glorot_net(ls, seed=11, beta=0.5)
    g = pkg.BP_GPU(1, 3, ls, B, 0.05, 0.5, 0.0, W, b, dropoutflag=1, visible_omit=0.1, hid_omit=0.2, seed=77,
                   max_chunk_frames=512)
    rng = np.random.default_rng(12)
    try:
        for ci in range(2):
            if ci == 1 and enhance:
                xs = WN.make_sentences(np.random.default_rng(13), [700, 300])
                g.enhance_waves(xs, np.zeros(FD, np.float32), np.ones(FD, np.float32), ctx, 1)
            n = 6 * B
            if windows:
                fea = rng.standard_normal((n + ctx - 1, FD)).astype(np.float32)
                tg = rng.standard_normal((n + ctx - 1, FD)).astype(np.float32)
                ws = np.arange(n, dtype=np.int32)
                g.train_windows(fea, tg, ctx, ws, ws + 1)
            else:
                g.train(n, rng.standard_normal((n, ctx * FD)).astype(np.float32), rng.standard_normal((n, FD)).astype(np.float32))
        return g.get_weights(), g.get_deltas()
    finally:
        g.close()


@pytest.mark.parametrize("windows", [False, True])
def test_training_unaffected_by_enhancement(pkg, windows):
    (w0, b0), (dw0, db0) = _train_pair(pkg, windows, False)
    (w1, b1), (dw1, db1) = _train_pair(pkg, windows, True)
    for l in (1, 2):
        for u, v in ((w0[l], w1[l]), (b0[l], b1[l]), (dw0[l], dw1[l]), (db0[l], db1[l])):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), l


# ---- argument checks that need a handle; the handle trains afterwards
def test_handle_argument_checks(pkg):
    ls = [3 * FD, 64, FD]
    W, b = pkg.glorot_net(ls, seed=1, beta=0.5)
    g = pkg.BP_GPU(1, 3, ls, 32, 0.05, 0.5, 0.0, W, b, max_chunk_frames=256)
    ref = pkg.BP_GPU(1, 3, ls, 32, 0.05, 0.5, 0.0, W, b, max_chunk_frames=256)
    xs = WN.make_sentences(np.random.default_rng(1), [400])
    mean, istd = np.zeros(FD, np.float32), np.ones(FD, np.float32)
    rng = np.random.default_rng(2)
    x, t = rng.standard_normal((64, 3 * FD)).astype(np.float32), rng.standard_normal((64, FD)).astype(np.float32)
    try:
        bad = [dict(context=3, targ_offset=0, out_col=1),              # out_col + fea_dim > sL
               dict(context=3, targ_offset=3, out_col=0),              # targ_offset outside [0, ctx)
               dict(context=3, targ_offset=-1, out_col=0),
               dict(context=4, targ_offset=0, out_col=0)]              # layersizes[0] is neither 4*D nor 5*D
        for kw in bad:
            with pytest.raises(pkg.BPError, match="status -1"):
                g.enhance_waves(xs, mean, istd, kw["context"], kw["targ_offset"], out_col=kw["out_col"])
        with pytest.raises(pkg.BPError, match="status -1"):           # more rows than the chunk capacity
            g.enhance_waves(WN.make_sentences(rng, [20000]), mean, istd, 3, 1)
        g.train(64, x, t)
        ref.train(64, x, t)
        (wg, bg), (wr, br) = g.get_weights(), ref.get_weights()
        for l in (1, 2):
            assert np.array_equal(wg[l], wr[l]) and np.array_equal(bg[l], br[l])
    finally:
        g.close()
        ref.close()


# ---- 9. the command-line tools end to end
def _write_pcm16(path, x, rate=8000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def _read_pcm16(path):
    import wave
    with wave.open(str(path), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2
        return np.frombuffer(w.readframes(w.getnframes()), np.int16).astype(np.float64), w.getframerate()


def _read_pfile(path, dim):
    raw = open(path, "rb").read()
    hdr = raw[:32768].split(b"\0")[0].decode()
    ns = int(hdr.split("-num_sentences")[1].split()[0]); nf = int(hdr.split("-num_frames")[1].split()[0])
    rec = np.frombuffer(raw, ">u4", nf * (2 + dim), 32768).reshape(nf, 2 + dim)
    table = np.frombuffer(raw, ">i4", ns + 1, 32768 + nf * (2 + dim) * 4)
    return rec[:, 0].astype(int), rec[:, 1].astype(int), rec[:, 2:].astype("<u4").view("<f4"), table


def _read_norm(path, dim):
    v = open(path).read().split("\n")
    return np.array(v[1:1 + dim], np.float64), np.array(v[2 + dim:2 + 2 * dim], np.float64)


def test_tools_end_to_end(pkg, tmp_path, parity_record):
    import subprocess
    import pfile_util as PU
    exe = {k: str(pkg.LIB_PATH).replace("libbp_hip.so", k) for k in ("bpfeat", "bpenhance", "bptrain")}
    rng = np.random.default_rng(9)
    lens = [4000, 1, 2500, 127, 3333, 6000, 800, 1500]
    noisy = [np.clip(x, -32768, 32767) for x in WN.make_sentences(rng, lens)]
    clean = [np.round(0.5 * x) for x in noisy]
    for tag, xs in (("noisy", noisy), ("clean", clean)):
        for s, x in enumerate(xs):
            _write_pcm16(tmp_path / ("%s%d.wav" % (tag, s)), x)
        (tmp_path / (tag + ".list")).write_text("".join("%s\n" % (tmp_path / ("%s%d.wav" % (tag, s))) for s in range(len(xs))))
        r = subprocess.run([exe["bpfeat"], "wav_list=%s" % (tmp_path / (tag + ".list")), "out_file=%s" % (tmp_path / (tag + ".pfile")),
                            "fea_dim=%d" % D, "norm_out=%s" % (tmp_path / (tag + ".norm"))], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1, r.stdout + r.stderr
    # records = the analysis of test 1 (same kernel: bit-equal), sentence structure from the WAV list
    sent, frame, fea, table = _read_pfile(tmp_path / "noisy.pfile", D)
    ref = pkg.wave_lps(0, D, noisy)
    assert np.array_equal(fea, np.concatenate(ref))
    assert list(np.diff(table)) == [r.shape[0] for r in ref]
    assert list(frame) == [t for r in ref for t in range(r.shape[0])]
    assert list(sent) == [s for s, r in enumerate(ref) for _ in range(r.shape[0])]
    m, i = _read_norm(tmp_path / "noisy.norm", D)
    L = np.concatenate(ref).astype(np.float64)
    e_norm = max(relerr(m, L.mean(0)), relerr(i, 1.0 / L.std(0)))
    assert e_norm <= 1e-5, e_norm
    # bptrain: one epoch on the noisy / clean pair
    ctx, toff = 3, 1
    ls = [ctx * D, 64, D]
    W, b = pkg.glorot_net(ls, seed=3, beta=0.5)
    PU.write_wts(str(tmp_path / "mlp.0.wts"), ls, W, b)
    args = ["fea_file=%s" % (tmp_path / "noisy.pfile"), "targ_file=%s" % (tmp_path / "clean.pfile"), "norm_file=%s" % (tmp_path / "noisy.norm"),
            "initwts_file=%s" % (tmp_path / "mlp.0.wts"), "outwts_file=%s" % (tmp_path / "mlp.1.wts"), "log_file=%s" % (tmp_path / "mlp.1.log"),
            "train_sent_range=0-5", "cv_sent_range=6-7", "fea_dim=%d" % D, "fea_context=%d" % ctx, "targ_offset=%d" % toff,
            "dropoutflag=0", "traincache=2000", "bunchsize=32", "gpu_used=1", "init_randem_seed=1", "momentum=0.5", "weightcost=0.0",
            "lrate=0.01", "visible_omit=0.0", "hid_omit=0.0", "numlayers=3", "layersizes=%s" % ",".join(map(str, ls))]
    r = subprocess.run([exe["bptrain"]] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "all finish!" in r.stdout, r.stdout + r.stderr
    # bpenhance with the identity net (as a .wts file) returns every input within 1 LSB
    m32, i32 = m.astype(np.float32), i.astype(np.float32)
    ls, W, b = WN.identity_net(D, 7, 3, True, m32, i32)
    PU.write_wts(str(tmp_path / "id.wts"), ls, W, b)
    (tmp_path / "enh.list").write_text("".join("%s %s\n" % (tmp_path / ("noisy%d.wav" % s), tmp_path / ("enh%d.wav" % s))
                                               for s in range(len(noisy))))
    r = subprocess.run([exe["bpenhance"], "norm_file=%s" % (tmp_path / "noisy.norm"), "initwts_file=%s" % (tmp_path / "id.wts"),
                        "layersizes=%s" % ",".join(map(str, ls)), "fea_dim=%d" % D, "fea_context=7", "targ_offset=3",
                        "wav_list=%s" % (tmp_path / "enh.list"), "traincache=60", "bunchsize=16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
    worst = 0.0
    for s, x in enumerate(noisy):
        y, rate = _read_pcm16(tmp_path / ("enh%d.wav" % s))
        assert rate == 8000 and y.size == x.size
        worst = max(worst, float(np.abs(y - x).max()))
    parity_record(norm_relerr=e_norm, enhance_max_lsb=worst)
    assert worst <= 1.0, worst
