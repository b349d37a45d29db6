"""GPU tests of the log-MMSE baseline (bp_logmmse_waves, bp_eval_mix_logmmse, bpenhance method=logmmse, bpeval baseline=logmmse;
-m gpu) against the float64 restatement in tests/classic_np.py and against the calls they are made of.

Bars: every VAD decision equals the restatement's, no exemptions (tests/test_classic_host.py holds every fixture sentence to a
margin of 1e-3 from the threshold, far above the analysis' fp32 error of about 1e-6); out_vad, out_pcm and G |Y_ref| within the
project's bar max|a - ref| / max|ref| < 1e-4 per sentence (tests/util.py); everything else bit for bit."""
import subprocess

import numpy as np
import pytest

import classic_np as CN
from util import TOL, relerr

pytestmark = pytest.mark.gpu
ALT = CN.ALT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(xs, ys):
    return len(xs) == len(ys) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(xs, ys))


def _against_restatement(D, kinds, xs, got, params):
    """{sentence: errors}; asserts the decisions and the bars."""
    pcm, gain, vad = got
    eta = params.get("eta", CN.DEFAULTS["eta"])
    errs = {}
    for i, (kind, x) in enumerate(zip(kinds, xs)):
        r = CN.reference(D, i, **params)
        assert gain[i].shape == r["G"].shape and vad[i].shape == r["vad"].shape and pcm[i].shape == x.shape
        assert np.array_equal(vad[i] < eta, r["noise"]), (D, kind, np.flatnonzero((vad[i] < eta) != r["noise"]))
        gy, gy_ref = gain[i].astype(np.float64) * r["absY"], r["G"] * r["absY"]
        e = dict(vad=relerr(vad[i], r["vad"]), pcm=relerr(pcm[i], r["pcm"]), gain_absY=relerr(gy, gy_ref))
        errs["%d:%s:%d" % (i, kind, x.size)] = e
        assert max(e.values()) < TOL, (D, kind, x.size, e)
        assert np.isfinite(pcm[i]).all() and np.isfinite(gain[i]).all() and np.isfinite(vad[i]).all()
        if kind == "zero":
            assert not pcm[i].any() and not gain[i].any()
    return errs


# ---- 1. bp_logmmse_waves against the restatement; the same bits on every run and in any company
@pytest.mark.parametrize("D", [33, 65, 129, 257])
def test_waves_match_restatement(pkg, D, parity_record):
    _, kinds, xs = [f for f in CN.fixtures() if f[0] == D][0]
    got = pkg.logmmse_waves(0, D, xs, return_gain=True, return_vad=True)
    parity_record(fea_dim=D, **_against_restatement(D, kinds, xs, got, {}))
    i = kinds.index("tones")
    parity_record(updates=int((got[2][i] < CN.DEFAULTS["eta"]).sum()), frames=int(got[2][i].size))
    again = pkg.logmmse_waves(0, D, xs, return_gain=True, return_vad=True)
    for a, b in zip(got, again):
        assert _same(a, b)
    assert _same(pkg.logmmse_waves(0, D, xs), got[0])               # without the optional outputs
    p, v = pkg.logmmse_waves(0, D, xs, return_vad=True)
    assert _same(p, got[0]) and _same(v, got[2])
    for i in range(len(xs)):                                      # a sentence alone = the same sentence in the batch
        p1, g1, v1 = pkg.logmmse_waves(0, D, [xs[i]], return_gain=True, return_vad=True)
        assert _same(p1, [got[0][i]]) and _same(g1, [got[1][i]]) and _same(v1, [got[2][i]]), (D, kinds[i])


def test_non_default_parameters(pkg, parity_record):
    D = 129
    _, kinds, xs = [f for f in CN.fixtures() if f[0] == D][0]
    dflt = pkg.logmmse_waves(0, D, xs)
    got = pkg.logmmse_waves(0, D, xs, ALT, return_gain=True, return_vad=True)
    assert not _same(got[0], dflt)
    parity_record(**_against_restatement(D, kinds, xs, got, ALT))
    lm = pkg.logmmse_params(ALT)                                  # a dict and the struct are the same call
    assert _same(pkg.logmmse_waves(0, D, xs, lm), got[0])
    assert _same(pkg.logmmse_waves(0, D, xs, dict(CN.DEFAULTS)), dflt)


def test_wide_spectrum_paths(pkg, parity_record):
    """fea_dim 513 and 1025 (3 and 5 bins per thread): the restatement's decisions and the bars, the same bits alone and in a batch."""
    for D, xs in CN.wide_fixtures():                              # (tests/test_classic_host.py vets sentence 0's VAD margin)
        p, g, v = pkg.logmmse_waves(0, D, xs, return_gain=True, return_vad=True)
        r = CN.enhance(xs[0], D)
        assert np.array_equal(v[0] < CN.DEFAULTS["eta"], r["noise"])
        e = dict(vad=relerr(v[0], r["vad"]), pcm=relerr(p[0], r["pcm"]), gain_absY=relerr(g[0].astype(np.float64) * r["absY"], r["G"] * r["absY"]))
        parity_record(**{"fea_dim_%d" % D: e})
        assert max(e.values()) < TOL, (D, e)
        p1, g1, v1 = pkg.logmmse_waves(0, D, [xs[2]], return_gain=True, return_vad=True)
        assert _same(p1, [p[2]]) and _same(g1, [g[2]]) and _same(v1, [v[2]])


# ---- 2. bp_eval_mix_logmmse is its parts
FS, D, CTX, TOFF = 8000, 129, 3, 1


def _corpus(rng):
    clean = [CN.gated_tones(s, n, D, 40.0, sigma=30.0) for s, n in ((21, 9000), (22, 6000), (23, 12000))]
    noise = [np.round(rng.normal(0, 800, 7000)).astype(np.float32), np.zeros(500, np.float32)]
    return clean, noise


def _plan(pkg):
    mixes = [(0, 0, 11, 0.0), (1, 1, 3, 5.0), (2, 0, 6999, 10.0), (1, 0, 100, -5.0)]    # (1, silent noise): g = 0, x == s
    p = np.zeros(len(mixes), pkg.MIXTURE_DTYPE)
    for i, m in enumerate(mixes):
        p[i] = m
    return p


def _handle(pkg, nat, bf16):
    ls = [(CTX + 1) * D if nat else CTX * D, 64, D]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    return pkg.BP_GPU(1, 3, ls, 32, 0.05, 0.5, 0.0, W, b, max_chunk_frames=1200, compute_dtype=int(bf16))


def _norm(rng):
    return rng.normal(10.0, 2.0, D).astype(np.float32), rng.uniform(0.2, 0.5, D).astype(np.float32)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("nat", [False, True])
def test_eval_mix_logmmse_is_its_parts(pkg, bf16, nat, parity_record):
    rng = np.random.default_rng(11)
    clean, noise = _corpus(rng)
    mean, istd = _norm(rng)
    plan = _plan(pkg)
    g = _handle(pkg, nat, bf16)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps")
        w0, d0 = g.get_weights(), g.get_deltas()
        ev = g.eval_mix_logmmse(plan, FS, return_pcm=True)
        w1, d1 = g.get_weights(), g.get_deltas()
        for a, b in zip(w0 + d0, w1 + d1):
            for x, y in zip(a, b):
                assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))
        lens = [clean[c].size for c in plan["clean"]]
        mix = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])
        enh = pkg.logmmse_waves(0, D, mix)
        refs = [clean[c] for c in plan["clean"]]
        assert _same(ev["pcm"], enh)
        assert np.array_equal(_bits(ev["noisy"]), _bits(pkg.score_waves(0, D, FS, refs, mix)))
        assert np.array_equal(_bits(ev["enhanced"]), _bits(pkg.score_waves(0, D, FS, refs, enh)))
        assert np.array_equal(_bits(ev["noisy"]), _bits(g.eval_mix(plan, FS)["noisy"]))
        alt = g.eval_mix_logmmse(plan, FS, ALT, return_pcm=True)
        assert _same(alt["pcm"], pkg.logmmse_waves(0, D, mix, ALT)) and not _same(alt["pcm"], enh)
        assert ev["pcm"] is not None and g.eval_mix_logmmse(plan, FS)["pcm"] is None
        # argument errors: BP_ERR_ARG, and the handle goes on as before
        for kw in ({"sample_rate": 44100}, {"params": {"alpha": 1.0}}, {"params": {"mu": 2.0}}, {"params": {"eta": float("nan")}},
                   {"params": {"xi_min_db": 1.0}}, {"params": {"gamma_max": 0.5}}, {"params": {"init_frames": 0}}):
            a = dict(sample_rate=FS)
            a.update(kw)
            with pytest.raises(pkg.BPError, match="status -1"):
                g.eval_mix_logmmse(plan, **a)
        bad = plan.copy()
        bad["clean"][0] = 99
        with pytest.raises(pkg.BPError, match="status -1"):
            g.eval_mix_logmmse(bad, FS)
        again = g.eval_mix_logmmse(plan, FS, return_pcm=True)
        assert _same(again["pcm"], enh) and np.array_equal(_bits(again["enhanced"]), _bits(ev["enhanced"]))
        parity_record(noisy=ev["noisy"].tolist(), logmmse=ev["enhanced"].tolist())
    finally:
        g.close()


def test_errors_leave_things_usable(pkg):
    x = CN.fixtures()[1][2][0]
    for kw in ({"fea_dim": 100}, {"fea_dim": 2049}, {"sentences": [x, np.zeros(0, np.float32)]}, {"params": {"alpha": -0.5}},
               {"params": {"mu": -1.0}}, {"params": {"eta": float("inf")}}, {"params": {"xi_min_db": -200.0}},
               {"params": {"gamma_max": float("inf")}}, {"params": {"init_frames": -3}}, {"device": 99}):
        a = dict(device=0, fea_dim=129, sentences=[x])
        a.update(kw)
        with pytest.raises(pkg.BPError, match="status -1"):
            pkg.logmmse_waves(**a)
    g = _handle(pkg, False, False)
    try:
        with pytest.raises(pkg.BPError, match="status -3"):      # no corpus
            g.eval_mix_logmmse(_plan(pkg), FS)
        rng = np.random.default_rng(11)
        clean, noise = _corpus(rng)
        g.set_mix_corpus(clean, noise, *_norm(rng), CTX, TOFF, "lps")
        assert np.isfinite(g.eval_mix_logmmse(_plan(pkg), FS)["enhanced"][:, 1]).all()
    finally:
        g.close()
    assert _same(pkg.logmmse_waves(0, 129, [x]), pkg.logmmse_waves(0, 129, [x]))


# ---- 3. the command-line tools
def _write_pcm16(path, x, rate):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def _read_pcm16(path):
    import wave
    with wave.open(str(path), "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), np.int16), w.getframerate()


def test_bpenhance_method_logmmse(pkg, tmp_path):
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpenhance")
    _, kinds, xs = CN.fixtures()[1]
    for i, x in enumerate(xs):
        _write_pcm16(tmp_path / ("in%d.wav" % i), x, FS)
    (tmp_path / "w.list").write_text("".join("%s %s\n" % (tmp_path / ("in%d.wav" % i), tmp_path / ("out%d.wav" % i)) for i in range(len(xs))))

    def run(*keys):
        return subprocess.run([exe, "method=logmmse", "fea_dim=129"] + list(keys), capture_output=True, text=True, timeout=120)
    r = run("wav_list=%s" % (tmp_path / "w.list"))
    assert r.returncode == 1 and "logmmse" in r.stdout, r.stdout + r.stderr
    want = pkg.logmmse_waves(0, 129, xs)
    for i in range(len(xs)):
        y, rate = _read_pcm16(tmp_path / ("out%d.wav" % i))
        assert rate == FS and np.array_equal(y, np.clip(np.rint(want[i]), -32768, 32767).astype(np.int16)), kinds[i]
    r = run("in_wav=%s" % (tmp_path / "in0.wav"), "out_wav=%s" % (tmp_path / "alt.wav"), "lm_alpha=0.95", "lm_mu=0.9", "lm_eta=0.2",
            "lm_xi_min_db=-15", "lm_gamma_max=20", "lm_init_frames=4")
    assert r.returncode == 1, r.stdout + r.stderr
    y, _ = _read_pcm16(tmp_path / "alt.wav")
    assert np.array_equal(y, np.clip(np.rint(pkg.logmmse_waves(0, 129, [xs[0]], ALT)[0]), -32768, 32767).astype(np.int16))
    # net keys, stream_block and bad values with it are errors: a message, exit status 0, nothing written
    io = ["in_wav=%s" % (tmp_path / "in0.wav"), "out_wav=%s" % (tmp_path / "no.wav")]
    for key in ("norm_file=x.norm", "initwts_file=a.wts", "layersizes=129,129", "fea_context=3", "stream_block=256", "wave_target=mask",
                "lm_alpha=1.5", "lm_init_frames=2.5", "lm_beta=1"):
        r = run(*(io + [key]))
        assert r.returncode == 0 and r.stdout.strip() and not (tmp_path / "no.wav").exists(), (key, r.stdout)
    r = subprocess.run([exe, "fea_dim=129", "lm_alpha=0.9"] + io, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "method=logmmse" in r.stdout


def test_bpeval_baseline_logmmse(pkg, tmp_path):
    import pfile_util as PU
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpeval")
    rng = np.random.default_rng(21)
    clean, noise = _corpus(rng)
    mean, istd = _norm(rng)
    for tag, xs in (("clean", clean), ("noise", noise)):
        for i, x in enumerate(xs):
            _write_pcm16(tmp_path / ("%s%d.wav" % (tag, i)), x, FS)
        (tmp_path / (tag + ".list")).write_text("".join("%s\n" % (tmp_path / ("%s%d.wav" % (tag, i))) for i in range(len(xs))))
    (tmp_path / "x.norm").write_text("<mean>\n" + "".join("%.9g\n" % v for v in mean) + "<inverse std>\n" +
                                     "".join("%.9g\n" % v for v in istd))
    ls = [CTX * D, 64, D]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    PU.write_wts(str(tmp_path / "net.wts"), ls, W, b)
    seed, snrs, per, cache = 77, [0.0, 10.0], 2, 400
    keys = ["clean_list=%s" % (tmp_path / "clean.list"), "noise_list=%s" % (tmp_path / "noise.list"), "norm_file=%s" % (tmp_path / "x.norm"),
            "initwts_file=%s" % (tmp_path / "net.wts"), "fea_dim=%d" % D, "fea_context=%d" % CTX, "targ_offset=%d" % TOFF,
            "layersizes=%s" % ",".join(map(str, ls)), "snr_list=0,10", "mix_per_clean=%d" % per, "init_randem_seed=%d" % seed,
            "traincache=%d" % cache, "bunchsize=32"]
    r0 = subprocess.run([exe] + keys + ["scores_out=%s" % (tmp_path / "s0.txt")], capture_output=True, text=True, timeout=300)
    r1 = subprocess.run([exe] + keys + ["scores_out=%s" % (tmp_path / "s1.txt"), "baseline=logmmse"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 1 and r1.returncode == 1, r0.stdout + r1.stdout + r1.stderr
    # with the key: every line of the run without it, each followed by its logmmse line; three more columns per mixture
    l0, l1 = r0.stdout.splitlines(), r1.stdout.splitlines()
    assert l1[0::2] == l0 and len(l1) == 2 * len(l0) == 6, r1.stdout
    for net, lm in zip(l1[0::2], l1[1::2]):                        # the same head and the same noisy SSNR
        assert lm.split(":")[0] == net.split(":")[0] and "logmmse: SSNR" in lm
        assert lm.split(" -> ")[0].split("SSNR ")[1] == net.split(" -> ")[0].split("SSNR ")[1]
    rows0 = [ln.split() for ln in open(tmp_path / "s0.txt").read().splitlines()]
    rows1 = [ln.split() for ln in open(tmp_path / "s1.txt").read().splitlines()]
    assert [r[:10] for r in rows1] == rows0 and all(len(r) == 13 for r in rows1)
    plan = pkg.mix_plan(seed, len(clean), per, [x.size for x in noise], snrs)
    g = pkg.BP_GPU(1, 3, ls, 32, 0.0, 0.0, 0.0, W, b, max_chunk_frames=cache)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps")
        T = g.mix_frames(plan) + CTX - 1                          # bpeval's cut: calls of at most traincache rows
        want, first, rows_ = [], 0, 0
        for i in range(len(plan) + 1):
            if i == len(plan) or rows_ + T[i] > cache:
                want.append(g.eval_mix_logmmse(plan[first:i], FS)["enhanced"])
                first, rows_ = i, 0
            if i < len(plan):
                rows_ += T[i]
        assert len(want) > 1
        want = np.concatenate(want)
    finally:
        g.close()
    assert [r[10:] for r in rows1] == [["%.9g" % v for v in w] for w in want]
    r = subprocess.run([exe, "pairs_list=%s" % (tmp_path / "clean.list"), "fea_dim=%d" % D, "baseline=logmmse"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "pairs_list takes only" in r.stdout
    r = subprocess.run([exe] + keys + ["baseline=wiener"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad value for baseline" in r.stdout
