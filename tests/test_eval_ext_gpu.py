"""GPU tests of the extended scores (bp_score_waves_ext, bp_eval_mix_ext, bp_eval_mix_logmmse_ext, bpeval scores=extended; -m gpu)
against the float64 restatement in tests/eval_ext_np.py and against the calls they are made of.  Bars: ESTOI 1e-4 absolute (the
project's STOI bar: the same fp32 front end; the restatement asserts that no STOI frame energy of a reference lies within 1 % of
its threshold, so the masks agree); SI-SDR 1e-4 dB (the project's SSNR bar: double accumulators on fp32 samples, only the order of
summation differs); columns 0..2 the bits of the three-column calls; bp_eval_mix_ext bit-identical to bp_mix_features + the
enhancer + bp_score_waves_ext.  tests/test_eval_ext_host.py shows that these bars catch a wrong formula."""
import functools
import math
import subprocess

import numpy as np
import pytest

import eval_ext_np as EX
import eval_np as EN
import test_eval_gpu as TE

pytestmark = pytest.mark.gpu
FS, D, CTX, TOFF = TE.FS, TE.D, TE.CTX, TE.TOFF
_bits = TE._bits


@functools.lru_cache(maxsize=None)
def _set(fs):
    """the pairs of eval_ext_np.pair_set at fs: made once, read only"""
    return EX.pair_set(np.random.default_rng(fs), fs)


# ---- 1. bp_score_waves_ext against the restatement
@pytest.mark.parametrize("fs", [8000, 16000, 48000])
def test_score_waves_ext_match_restatement(pkg, fs, parity_record):
    refs, ests = _set(fs)
    got = pkg.score_waves(0, D, fs, refs, ests, extended=True)
    assert got.shape == (len(refs), 5) and got.dtype == np.float32
    err = {"estoi_abs": 0.0, "sisdr_db": 0.0}
    for i, (r, e) in enumerate(zip(refs, ests)):
        err["estoi_abs"] = max(err["estoi_abs"], abs(float(got[i, pkg.SCORE_ESTOI]) - EX.estoi(r, e, fs, check_margin=True)))
        err["sisdr_db"] = max(err["sisdr_db"], abs(float(got[i, pkg.SCORE_SISDR]) - EX.sisdr(r, e)))
    print(fs, err, got[:, 3:].tolist())
    parity_record(fs=fs, estoi=got[:, 3].tolist(), sisdr=got[:, 4].tolist(), **err)
    assert err["estoi_abs"] <= 1e-4 and err["sisdr_db"] <= 1e-4, err
    assert np.all(np.diff(got[:3, pkg.SCORE_ESTOI]) > 0) and np.all(np.diff(got[:3, pkg.SCORE_SISDR]) > 0), got   # rise with the SNR


# ---- 2. the three columns stay; the same bits on every run
@pytest.mark.parametrize("fs", [8000, 16000])
def test_ext_columns_0_to_2_are_score_waves(pkg, fs):
    refs, ests = _set(fs)
    five = pkg.score_waves(0, D, fs, refs, ests, extended=True)
    three = pkg.score_waves(0, D, fs, refs, ests)
    assert three.shape == (len(refs), 3)
    assert np.array_equal(_bits(five[:, :3]), _bits(three))
    assert np.array_equal(_bits(five), _bits(pkg.score_waves(0, D, fs, refs, ests, extended=True)))
    one = pkg.score_waves(0, D, fs, refs[2:3], ests[2:3], extended=True)            # a pair alone = the pair in the batch
    assert np.array_equal(_bits(one[0]), _bits(five[2]))


# ---- 3. edge cases
def test_score_waves_ext_edge_cases(pkg, parity_record):
    fs = 16000
    rng = np.random.default_rng(7)
    r = EN.speech_like(rng, 3 * fs, fs, gaps=0)
    silent = np.zeros(fs, np.float32)
    short = EN.speech_like(rng, int(0.3 * fs), fs, gaps=0)    # < 31 STOI frames at 10 kHz
    tiny = EN.speech_like(rng, 400, fs, gaps=0)
    one = np.array([1234.0], np.float32)
    refs = [r, r, silent, short, tiny, one, r]
    ests = [r.copy(), 3 * r, EN.add_noise(rng, r[:fs], 5.0), EN.add_noise(rng, short, 5.0), EN.add_noise(rng, tiny, 5.0),
            np.array([-77.0], np.float32), np.zeros_like(r)]
    got = pkg.score_waves(0, D, fs, refs, ests, extended=True)
    es, sd = got[:, pkg.SCORE_ESTOI], got[:, pkg.SCORE_SISDR]
    parity_record(estoi=es.tolist(), sisdr=sd.tolist())
    assert abs(es[0] - 1.0) <= 1e-6 and sd[0] >= 100.0, got[0]
    assert abs(es[1] - 1.0) <= 1e-5 and sd[1] >= 100.0, got[1]
    assert np.isnan(es[2]) and np.isnan(sd[2]), got[2]
    assert np.isnan(es[3]) and np.isfinite(sd[3]), got[3]
    assert np.isnan(es[4]) and np.isfinite(sd[4]), got[4]
    assert np.isnan(es[5]) and np.isfinite(sd[5]), got[5]
    assert es[6] == 0.0 and abs(sd[6] - 10 * math.log10(EX.EPS)) <= 1e-4, got[6]
    assert np.array_equal(_bits(got[:, :3]), _bits(pkg.score_waves(0, D, fs, refs, ests)))
    assert np.array_equal(_bits(got), _bits(pkg.score_waves(0, D, fs, refs, ests, extended=True)))


# ---- 4. bp_eval_mix_ext and bp_eval_mix_logmmse_ext are their parts
@pytest.mark.parametrize("bf16", [False, True])
def test_eval_mix_ext_is_its_parts(pkg, bf16, parity_record):
    rng = np.random.default_rng(11)
    clean, noise = TE._corpus(rng)
    mean, istd = TE._norm(rng)
    plan = TE._plan(pkg)
    g = TE._handle(pkg, False, bf16)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps+irm")
        ev = g.eval_mix(plan, FS, pkg.WAVE_MASK, D, return_pcm=True, extended=True)
        lm = g.eval_mix_logmmse(plan, FS, return_pcm=True, extended=True)
        assert ev["noisy"].shape == ev["enhanced"].shape == lm["enhanced"].shape == (len(plan), 5)
        lens = [clean[c].size for c in plan["clean"]]
        mix = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])
        refs = [clean[c] for c in plan["clean"]]
        enh = g.enhance_waves(mix, mean, istd, CTX, TOFF, pkg.WAVE_MASK, D)
        lmw = pkg.logmmse_waves(0, D, mix)
        for a, b in zip(ev["pcm"], enh):
            assert np.array_equal(_bits(a), _bits(b))
        for a, b in zip(lm["pcm"], lmw):
            assert np.array_equal(_bits(a), _bits(b))
        noisy = pkg.score_waves(0, D, FS, refs, mix, extended=True)
        assert np.array_equal(_bits(ev["noisy"]), _bits(noisy)) and np.array_equal(_bits(lm["noisy"]), _bits(noisy))
        assert np.array_equal(_bits(ev["enhanced"]), _bits(pkg.score_waves(0, D, FS, refs, enh, extended=True)))
        assert np.array_equal(_bits(lm["enhanced"]), _bits(pkg.score_waves(0, D, FS, refs, lmw, extended=True)))
        # columns 0..2: the three-column calls
        ev3, lm3 = g.eval_mix(plan, FS, pkg.WAVE_MASK, D), g.eval_mix_logmmse(plan, FS)
        assert ev3["noisy"].shape == (len(plan), 3)
        for k in ("noisy", "enhanced"):
            assert np.array_equal(_bits(ev[k][:, :3]), _bits(ev3[k])) and np.array_equal(_bits(lm[k][:, :3]), _bits(lm3[k]))
        # mixture 1 has a silent noise: x == s
        assert abs(ev["noisy"][1, pkg.SCORE_ESTOI] - 1.0) <= 1e-6 and ev["noisy"][1, pkg.SCORE_SISDR] >= 100.0, ev["noisy"][1]
        with pytest.raises(pkg.BPError, match="status -1"):
            g.eval_mix(plan, 44100, pkg.WAVE_MASK, D, extended=True)
        parity_record(noisy=ev["noisy"].tolist(), enhanced=ev["enhanced"].tolist(), logmmse=lm["enhanced"].tolist())
    finally:
        g.close()


# ---- 5. bpeval scores=extended
def _rows(path):
    return [ln.split() for ln in open(path).read().splitlines()]


def _fmt(a):
    return [["%.9g" % v for v in row] for row in a]


def test_bpeval_scores_extended(pkg, tmp_path):
    import pfile_util as PU
    exe = str(pkg.LIB_PATH).replace("libbp_hip.so", "bpeval")
    rng = np.random.default_rng(21)
    clean, noise = TE._corpus(rng)
    mean, istd = TE._norm(rng)
    for tag, xs in (("clean", clean), ("noise", noise)):
        for i, x in enumerate(xs):
            TE._write_pcm16(tmp_path / ("%s%d.wav" % (tag, i)), x, FS)
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
            "traincache=%d" % cache, "bunchsize=32", "baseline=logmmse"]
    r0 = subprocess.run([exe] + keys + ["scores_out=%s" % (tmp_path / "s0.txt"), "scores=basic"], capture_output=True, text=True, timeout=300)
    r1 = subprocess.run([exe] + keys + ["scores_out=%s" % (tmp_path / "s1.txt"), "scores=extended"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 1 and r1.returncode == 1, r0.stdout + r1.stdout + r1.stderr
    # stdout: the basic line up to its STOI figures, then the two new scores, then the undefined count
    l0, l1 = r0.stdout.splitlines(), r1.stdout.splitlines()
    assert len(l0) == len(l1) == 6, r1.stdout
    for basic, ext in zip(l0, l1):
        head, tail = ext.split(", ESTOI ")
        assert basic.startswith(head + " (") and "ESTOI" not in basic, (basic, ext)
        est, rest = tail.split(", SI-SDR ")
        assert len(est.split(" -> ")) == 2 and rest.split(" dB (")[1].endswith(" undefined)") and len(rest.split(" dB (")[0].split(" -> ")) == 2, ext
    rows0, rows1 = _rows(tmp_path / "s0.txt"), _rows(tmp_path / "s1.txt")
    assert all(len(r) == 13 for r in rows0) and all(len(r) == 19 for r in rows1)
    assert [r[:10] for r in rows1] == [r[:10] for r in rows0] and [r[14:17] for r in rows1] == [r[10:] for r in rows0]
    plan = pkg.mix_plan(seed, len(clean), per, [x.size for x in noise], snrs)
    g = pkg.BP_GPU(1, 3, ls, 32, 0.0, 0.0, 0.0, W, b, max_chunk_frames=cache)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps")
        T = g.mix_frames(plan) + CTX - 1                          # bpeval's cut: calls of at most traincache rows
        net, lmm, first, rows_ = [], [], 0, 0
        for i in range(len(plan) + 1):
            if i == len(plan) or rows_ + T[i] > cache:
                ev = g.eval_mix(plan[first:i], FS, extended=True)
                net.append(np.stack([ev["noisy"][:, 3], ev["enhanced"][:, 3], ev["noisy"][:, 4], ev["enhanced"][:, 4]], axis=1))
                lmm.append(g.eval_mix_logmmse(plan[first:i], FS, extended=True)["enhanced"][:, 3:])
                first, rows_ = i, 0
            if i < len(plan):
                rows_ += T[i]
        assert len(net) > 1
    finally:
        g.close()
    assert [r[10:14] for r in rows1] == _fmt(np.concatenate(net))
    assert [r[17:] for r in rows1] == _fmt(np.concatenate(lmm))
    # pairs mode
    refs = [clean[0], clean[3]]
    ests = [np.round(EN.add_noise(rng, x, 3.0)).clip(-32768, 32767).astype(np.float32) for x in refs]
    lines = []
    for i, (x, y) in enumerate(zip(refs, ests)):
        TE._write_pcm16(tmp_path / ("r%d.wav" % i), x, FS)
        TE._write_pcm16(tmp_path / ("e%d.wav" % i), y, FS)
        lines.append("%s %s\n" % (tmp_path / ("r%d.wav" % i), tmp_path / ("e%d.wav" % i)))
    (tmp_path / "p.list").write_text("".join(lines))
    pk = [exe, "pairs_list=%s" % (tmp_path / "p.list"), "fea_dim=%d" % D]
    p0 = subprocess.run(pk + ["scores_out=%s" % (tmp_path / "p0.txt"), "scores=basic"], capture_output=True, text=True, timeout=300)
    p1 = subprocess.run(pk + ["scores_out=%s" % (tmp_path / "p1.txt"), "scores=extended"], capture_output=True, text=True, timeout=300)
    assert p0.returncode == 1 and p1.returncode == 1, p0.stdout + p1.stdout + p1.stderr
    head, tail = p1.stdout.split(", ESTOI ")
    assert p0.stdout.startswith(head + " (") and ", SI-SDR " in tail and tail.endswith(" dB (0 undefined)\n"), (p0.stdout, p1.stdout)
    q0, q1 = _rows(tmp_path / "p0.txt"), _rows(tmp_path / "p1.txt")
    assert [r[:5] for r in q1] == q0 and all(len(r) == 7 for r in q1)
    assert [r[2:] for r in q1] == _fmt(pkg.score_waves(0, D, FS, refs, ests, extended=True))
