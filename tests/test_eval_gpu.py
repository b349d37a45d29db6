"""GPU tests of the objective scores (bp_score_waves, bp_eval_mix, bpeval; -m gpu) against the float64 restatement in
tests/eval_np.py and against the calls they are made of.  Bars: SSNR 1e-4 dB; LSD 1e-3 relative to the restatement and 1e-5
relative to the float64 formula on bp_wave_lps; STOI 1e-4 absolute (the restatement asserts that no STOI frame energy of a
reference lies within 1 % of its threshold, so the masks agree); bp_eval_mix bit-identical to bp_mix_features +
bp_enhance_waves + bp_score_waves."""
import subprocess

import numpy as np
import pytest

import eval_np as EN

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set(rng, fs, D):
    """references with gaps and a floor; estimates: white noise at 0, 10 and 20 dB, one pair per length"""
    refs = [EN.speech_like(rng, int(sec * fs), fs) for sec in (3.0, 2.5, 4.0)]
    ests = [EN.add_noise(rng, r, snr) for r, snr in zip(refs, (0.0, 10.0, 20.0))]
    return refs, ests


# ---- 1. bp_score_waves against the restatement
@pytest.mark.parametrize("fs", [8000, 10000, 16000, 48000])
@pytest.mark.parametrize("D", [129, 257])
def test_score_waves_match_restatement(pkg, fs, D, parity_record):
    score_case(pkg, fs, D, parity_record)


def score_case(pkg, fs, D, parity_record):
    """The body of test_score_waves_match_restatement (tests/test_geometry_gpu.py runs it at the other frame sizes)."""
    rng = np.random.default_rng(fs + D)
    refs, ests = _set(rng, fs, D)
    got = pkg.score_waves(0, D, fs, refs, ests)
    lps = pkg.wave_lps(0, D, refs + ests)
    err = {"ssnr_db": 0.0, "lsd_rel": 0.0, "lsd_rel_gpu_lps": 0.0, "stoi_abs": 0.0}
    for i, (r, e) in enumerate(zip(refs, ests)):
        want = EN.scores(r, e, fs, D, check_margin=True)
        err["ssnr_db"] = max(err["ssnr_db"], abs(float(got[i, 0]) - want[0]))
        err["lsd_rel"] = max(err["lsd_rel"], abs(float(got[i, 1]) - want[1]) / want[1])
        l64 = EN.lsd_of_lps(lps[i], lps[len(refs) + i])
        err["lsd_rel_gpu_lps"] = max(err["lsd_rel_gpu_lps"], abs(float(got[i, 1]) - l64) / l64)
        err["stoi_abs"] = max(err["stoi_abs"], abs(float(got[i, 2]) - want[2]))
    parity_record(fea_dim=D, **err)
    assert err["ssnr_db"] <= 1e-4 and err["lsd_rel"] <= 1e-3 and err["lsd_rel_gpu_lps"] <= 1e-5 and err["stoi_abs"] <= 1e-4, err
    assert np.all(np.diff(got[:, 2]) > 0)                     # STOI rises with the SNR


# ---- 2. edge cases
def test_score_waves_edge_cases(pkg, parity_record):
    fs, D = 16000, 129
    rng = np.random.default_rng(7)
    r = EN.speech_like(rng, 3 * fs, fs, gaps=0)               # no all-zero SSNR frame
    silent = np.zeros(fs, np.float32)
    short = EN.speech_like(rng, int(0.3 * fs), fs, gaps=0)    # < 31 STOI frames at 10 kHz
    tiny = EN.speech_like(rng, 400, fs, gaps=0)               # < one SSNR frame (win = 480)
    one = np.array([1234.0], np.float32)
    refs = [r, r, silent, short, tiny, one]
    ests = [r.copy(), 3 * r, EN.add_noise(rng, r[:fs], 5.0), EN.add_noise(rng, short, 5.0), EN.add_noise(rng, tiny, 5.0),
            np.array([-77.0], np.float32)]
    got = pkg.score_waves(0, D, fs, refs, ests)
    parity_record(identity=got[0].tolist(), scaled_stoi=float(got[1, 2]))
    assert got[0, 0] == 35.0 and got[0, 1] == 0.0 and abs(got[0, 2] - 1.0) <= 1e-6, got[0]
    assert abs(got[1, 2] - 1.0) <= 1e-5, got[1]
    assert got[2, 0] == -10.0 and np.isnan(got[2, 2]), got[2]
    assert np.isfinite(got[3, 0]) and np.isnan(got[3, 2]), got[3]
    assert np.isnan(got[4, 0]) and np.isnan(got[4, 2]) and np.isfinite(got[4, 1]), got[4]
    assert np.isnan(got[5, 0]) and np.isnan(got[5, 2]) and np.isfinite(got[5, 1]), got[5]
    assert got[5, 1] == pytest.approx(EN.lsd_of_lps(*pkg.wave_lps(0, D, [one, ests[5]])), rel=1e-5)
    again = pkg.score_waves(0, D, fs, refs, ests)
    assert np.array_equal(_bits(got), _bits(again))


# ---- 3. bp_eval_mix
FS, D, CTX, TOFF = 8000, 129, 3, 1


def _corpus(rng):
    clean = [np.round(EN.speech_like(rng, n, FS, gaps=g)) for n, g in ((24000, 2), (20000, 0), (30000, 1), (9000, 0))]
    noise = [np.round(rng.normal(0, 2000, 7000)).astype(np.float32), np.zeros(500, np.float32),
             np.round(rng.normal(0, 500, 40000)).astype(np.float32)]
    return [c.astype(np.float32) for c in clean], noise


def _plan(pkg):
    mixes = [(0, 0, 11, 0.0), (1, 1, 3, 5.0),                 # (1, silent noise): g = 0, x == s
             (2, 2, 39000, 10.0), (3, 0, 6999, -5.0), (1, 2, 100, 20.0)]
    p = np.zeros(len(mixes), pkg.MIXTURE_DTYPE)
    for i, m in enumerate(mixes):
        p[i] = m
    return p


def _handle(pkg, nat, bf16):
    ls = [(CTX + 1) * D if nat else CTX * D, 64, 2 * D]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    return pkg.BP_GPU(1, 3, ls, 32, 0.05, 0.5, 0.0, W, b, max_chunk_frames=3000, compute_dtype=int(bf16))


def _norm(rng):
    return rng.normal(10.0, 2.0, D).astype(np.float32), rng.uniform(0.2, 0.5, D).astype(np.float32)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("nat", [False, True])
@pytest.mark.parametrize("target", [0, 1])
def test_eval_mix_is_its_parts(pkg, bf16, nat, target, parity_record):
    rng = np.random.default_rng(11)
    clean, noise = _corpus(rng)
    mean, istd = _norm(rng)
    plan = _plan(pkg)
    out_col = 0 if target == pkg.WAVE_LPS else D
    g, ref = _handle(pkg, nat, bf16), _handle(pkg, nat, bf16)
    try:
        for h in (g, ref):
            h.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps+irm")
        w0, d0 = g.get_weights(), g.get_deltas()
        ev = g.eval_mix(plan, FS, target, out_col, return_pcm=True)
        w1, d1 = g.get_weights(), g.get_deltas()
        for a, b in zip(w0 + d0, w1 + d1):
            for x, y in zip(a, b):
                assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))
        # the parts: the mixtures of bp_mix_features, bp_enhance_waves on them, bp_score_waves
        lens = [clean[c].size for c in plan["clean"]]
        mix = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])
        enh = g.enhance_waves(mix, mean, istd, CTX, TOFF, target, out_col)
        refs = [clean[c] for c in plan["clean"]]
        for a, b in zip(ev["pcm"], enh):
            assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(ev["noisy"]), _bits(pkg.score_waves(0, D, FS, refs, mix)))
        assert np.array_equal(_bits(ev["enhanced"]), _bits(pkg.score_waves(0, D, FS, refs, enh)))
        assert ev["noisy"][1, 0] == 35.0 and abs(ev["noisy"][1, 2] - 1.0) <= 1e-6, ev["noisy"][1]
        # bad arguments: BP_ERR_ARG, the handle unchanged
        for kw in ({"sample_rate": 44100}, {"target": 2}, {"out_col": D + 1}, {"out_col": -1}):
            a = dict(sample_rate=FS, target=target, out_col=out_col)
            a.update(kw)
            with pytest.raises(pkg.BPError, match="status -1"):
                g.eval_mix(plan, **a)
        # training afterwards is unaffected
        g.train_mix(plan)
        ref.train_mix(plan)
        for x, y in zip(g.get_weights()[0], ref.get_weights()[0]):
            assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))
        parity_record(noisy=ev["noisy"].tolist(), enhanced=ev["enhanced"].tolist())
    finally:
        g.close()
        ref.close()


def test_eval_mix_needs_a_corpus(pkg):
    g = _handle(pkg, False, False)
    try:
        with pytest.raises(pkg.BPError, match="status -3"):
            g.eval_mix(_plan(pkg), FS)
    finally:
        g.close()


# ---- 4. bpeval
def _write_pcm16(path, x, rate):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def _read_scores(path, skip):
    rows = [ln.split() for ln in open(path).read().splitlines()]
    return rows, np.array([[float(v) for v in r[skip:]] for r in rows], np.float32)


def test_bpeval_matches_the_calls(pkg, tmp_path):
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
    ls = [CTX * D, 64, 2 * D]
    W, b = pkg.glorot_net(ls, seed=5, beta=0.5)
    PU.write_wts(str(tmp_path / "net.wts"), ls, W, b)
    seed, snrs, per = 77, [-5.0, 0.0, 5.0], 2
    r = subprocess.run([exe, "clean_list=%s" % (tmp_path / "clean.list"), "noise_list=%s" % (tmp_path / "noise.list"),
                        "norm_file=%s" % (tmp_path / "x.norm"), "initwts_file=%s" % (tmp_path / "net.wts"), "fea_dim=%d" % D,
                        "fea_context=%d" % CTX, "targ_offset=%d" % TOFF, "layersizes=%s" % ",".join(map(str, ls)),
                        "snr_list=-5,0,5", "mix_per_clean=%d" % per, "init_randem_seed=%d" % seed, "traincache=1200",
                        "bunchsize=32", "wave_target=mask", "out_col=%d" % D, "scores_out=%s" % (tmp_path / "s.txt")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["SNR -5 dB", "SNR 0 dB", "SNR 5 dB", "all"], r.stdout
    plan = pkg.mix_plan(seed, len(clean), per, [x.size for x in noise], snrs)
    rows, got = _read_scores(tmp_path / "s.txt", 4)
    assert [(int(a), int(b), int(c), float(d)) for a, b, c, d, *_ in rows] == \
        [(int(m["clean"]), int(m["noise"]), int(m["offset"]), float(m["snr_db"])) for m in plan]
    g = pkg.BP_GPU(1, 3, ls, 32, 0.0, 0.0, 0.0, W, b, max_chunk_frames=1200)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps+irm")
        T = g.mix_frames(plan) + CTX - 1                      # bpmix's cut: calls of at most traincache rows
        want, first, rows_ = [], 0, 0
        for i in range(len(plan) + 1):
            if i == len(plan) or rows_ + T[i] > 1200:
                ev = g.eval_mix(plan[first:i], FS, pkg.WAVE_MASK, D)
                want.append(np.stack([ev["noisy"][:, 0], ev["enhanced"][:, 0], ev["noisy"][:, 1], ev["enhanced"][:, 1],
                                      ev["noisy"][:, 2], ev["enhanced"][:, 2]], axis=1))
                first, rows_ = i, 0
            if i < len(plan):
                rows_ += T[i]
        assert len(want) > 1                                  # (the plan needed more than one call)
        assert np.array_equal(_bits(got), _bits(np.concatenate(want)))
    finally:
        g.close()
    # pairs mode
    refs = [clean[0], clean[3]]
    ests = [np.round(EN.add_noise(rng, x, 3.0)).clip(-32768, 32767).astype(np.float32) for x in refs]
    lines = []
    for i, (x, y) in enumerate(zip(refs, ests)):
        _write_pcm16(tmp_path / ("r%d.wav" % i), x, FS)
        _write_pcm16(tmp_path / ("e%d.wav" % i), y, FS)
        lines.append("%s %s\n" % (tmp_path / ("r%d.wav" % i), tmp_path / ("e%d.wav" % i)))
    (tmp_path / "p.list").write_text("".join(lines))
    r = subprocess.run([exe, "pairs_list=%s" % (tmp_path / "p.list"), "fea_dim=%d" % D, "scores_out=%s" % (tmp_path / "p.txt")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith("pairs: 2 pairs"), r.stdout + r.stderr
    _, got = _read_scores(tmp_path / "p.txt", 2)
    assert np.array_equal(_bits(got), _bits(pkg.score_waves(0, D, FS, refs, ests)))
