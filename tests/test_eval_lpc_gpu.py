"""GPU tests of the spectral-envelope scores LLR and cepstral distance (the _ext calls with seven columns, extended="full",
bpeval scores=full; -m gpu) against the float64 restatement in tests/eval_lpc_np.py and against the calls they are made of.

Bars, absolute: LLR 1e-5, CD 1e-4 dB.  The fp32 rounding of a result in [0, 2] / [0, 10] is 1.2e-7 / 6e-7; the order of the
double operations moves a frame value by at most (P+1) 1e6 2^-53 = 2e-9 (the condition the white-noise correction guarantees),
and float64 against 80-bit arithmetic differs by at most 2.2e-12 on these fixtures (tests/test_eval_lpc_host.py): both bars leave
more than 10 x over that, and 1e-4 dB is the bar SI-SDR has.  The NaN pattern must be equal.  tests/test_eval_lpc_host.py shows
that these bars catch a wrong formula.  Everything else is bit for bit: the same bits on every run and in any company, columns
0..4 the five-column call, the five- and three-column calls untouched by a seven-column call before them, and the eval_mix
calls equal to score_waves on their own audio."""
import functools
import subprocess

import numpy as np
import pytest

import eval_lpc_np as LP
import test_eval_gpu as TE

pytestmark = pytest.mark.gpu
FS, D, CTX, TOFF = TE.FS, TE.D, TE.CTX, TE.TOFF
_bits = TE._bits
FEA = {8000: 129, 16000: 257}


@functools.lru_cache(maxsize=None)
def _set(fs):
    """(names, refs, ests, want [n][2]) of eval_lpc_np.fixtures() at fs, the restatement's scores beside them: made once, read only"""
    fx = {k: v for k, v in LP.fixtures().items() if v[0] == fs}
    names = sorted(fx)
    refs, ests = [fx[k][1] for k in names], [fx[k][2] for k in names]
    want = np.array([LP.llr_cd(r, e, fs) for r, e in zip(refs, ests)], np.float64)
    return names, refs, ests, want


# ---- 1. against the restatement
@pytest.mark.parametrize("fs", [8000, 16000])
def test_score_waves_full_match_restatement(pkg, fs, parity_record):
    names, refs, ests, want = _set(fs)
    got = pkg.score_waves(0, FEA[fs], fs, refs, ests, extended="full")
    assert got.shape == (len(refs), 7) and got.dtype == np.float32
    llr, cd = got[:, pkg.SCORE_LLR].astype(np.float64), got[:, pkg.SCORE_CD].astype(np.float64)
    nan = np.isnan(want)
    err = {"llr_abs": float(np.nanmax(np.abs(llr - want[:, 0]))), "cd_db": float(np.nanmax(np.abs(cd - want[:, 1])))}
    print(fs, err)
    for k, name in enumerate(names):
        print("  %-11s LLR %.7f (%.7f)  CD %.6f (%.6f)" % (name, llr[k], want[k, 0], cd[k], want[k, 1]))
    parity_record(fs=fs, names=names, llr=llr.tolist(), cd=cd.tolist(), bar_llr=LP.BAR_LLR, bar_cd_db=LP.BAR_CD, **err)
    assert np.array_equal(np.isnan(llr), nan[:, 0]) and np.array_equal(np.isnan(cd), nan[:, 1]), (names, got[:, 5:])
    assert nan[:, 0].sum() == 3 and (~nan[:, 0]).sum() == 10                   # zeros, short, noframe; everything else is scored
    assert err["llr_abs"] <= LP.BAR_LLR and err["cd_db"] <= LP.BAR_CD, err


@functools.lru_cache(maxsize=None)
def _set_80k():
    """two short pairs at 80 kHz: the frame of 2400 samples is longer than the kernel keeps in LDS, so its lag sums take
    their other path"""
    fs = 80000
    rng = np.random.default_rng(4300)
    r = LP.speech_like(rng, fs, sec=0.4)
    refs, ests = [r, r[:fs // 8]], [LP.reverberate(rng, r, fs, 50.0), LP.add_noise(rng, r[:fs // 8], 30.0)]
    return fs, refs, ests, np.array([LP.llr_cd(x, y, fs) for x, y in zip(refs, ests)], np.float64)


def test_score_waves_full_long_frames(pkg, parity_record):
    fs, refs, ests, want = _set_80k()
    got = pkg.score_waves(0, 257, fs, refs, ests, extended="full").astype(np.float64)
    err = {"llr_abs": float(np.abs(got[:, 5] - want[:, 0]).max()), "cd_db": float(np.abs(got[:, 6] - want[:, 1]).max())}
    print(fs, err, got[:, 5:].tolist(), want.tolist())
    parity_record(fs=fs, llr=got[:, 5].tolist(), cd=got[:, 6].tolist(), **err)
    assert np.all(np.isfinite(want)) and np.all(want > 0.0)
    assert err["llr_abs"] <= LP.BAR_LLR and err["cd_db"] <= LP.BAR_CD, err


# ---- 2. bit for bit
@pytest.mark.parametrize("fs", [8000, 16000])
def test_full_columns_and_company(pkg, fs):
    names, refs, ests, _ = _set(fs)
    D_ = FEA[fs]
    three0, five0 = pkg.score_waves(0, D_, fs, refs, ests), pkg.score_waves(0, D_, fs, refs, ests, extended=True)
    seven = pkg.score_waves(0, D_, fs, refs, ests, extended="full")
    assert np.array_equal(_bits(seven), _bits(pkg.score_waves(0, D_, fs, refs, ests, extended="full")))      # two calls, the same bits
    assert np.array_equal(_bits(seven[:, :5]), _bits(five0))                                                # columns 0..4: the five-column call
    # the five- and three-column calls after a seven-column call are what they were before it
    assert np.array_equal(_bits(pkg.score_waves(0, D_, fs, refs, ests, extended=True)), _bits(five0))
    assert np.array_equal(_bits(pkg.score_waves(0, D_, fs, refs, ests)), _bits(three0))
    # a pair alone equals the same pair among five others
    k = names.index("burst" + ("8" if fs == 8000 else "16"))
    others = [i for i in range(len(names)) if i != k][:5]
    mixed = others[:2] + [k] + others[2:]
    alone = pkg.score_waves(0, D_, fs, [refs[k]], [ests[k]], extended="full")
    among = pkg.score_waves(0, D_, fs, [refs[i] for i in mixed], [ests[i] for i in mixed], extended="full")
    assert np.array_equal(_bits(alone[0]), _bits(among[2])) and np.array_equal(_bits(alone[0]), _bits(seven[k]))


def test_eval_mix_full_is_score_waves_on_its_own_audio(pkg, parity_record):
    rng = np.random.default_rng(11)
    clean, noise = TE._corpus(rng)
    mean, istd = TE._norm(rng)
    plan = TE._plan(pkg)
    g = TE._handle(pkg, False, False)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps+irm")
        five = g.eval_mix(plan, FS, pkg.WAVE_MASK, D, extended=True)
        ev = g.eval_mix(plan, FS, pkg.WAVE_MASK, D, return_pcm=True, extended="full")
        lm = g.eval_mix_logmmse(plan, FS, return_pcm=True, extended="full")
        sp = g.eval_mix_logmmse(plan, FS, return_pcm=True, extended="full", noise="spp")
        lens = [clean[c].size for c in plan["clean"]]
        mix = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])
        refs = [clean[c] for c in plan["clean"]]
        noisy = pkg.score_waves(0, D, FS, refs, mix, extended="full")
        for out in (ev, lm, sp):
            assert out["noisy"].shape == out["enhanced"].shape == (len(plan), 7)
            assert np.array_equal(_bits(out["noisy"]), _bits(noisy))
            assert np.array_equal(_bits(out["enhanced"]), _bits(pkg.score_waves(0, D, FS, refs, out["pcm"], extended="full")))
        assert not np.array_equal(_bits(lm["enhanced"]), _bits(sp["enhanced"]))
        # columns 0..4, and the five-column call after the seven-column ones
        again = g.eval_mix(plan, FS, pkg.WAVE_MASK, D, extended=True)
        for k in ("noisy", "enhanced"):
            assert np.array_equal(_bits(ev[k][:, :5]), _bits(five[k])) and np.array_equal(_bits(again[k]), _bits(five[k]))
        # mixture 1 has a silent noise: x == s
        assert ev["noisy"][1, pkg.SCORE_LLR] == 0.0 and ev["noisy"][1, pkg.SCORE_CD] == 0.0, ev["noisy"][1]
        assert np.all(np.isfinite(ev["noisy"][:, 5:])) and np.all(ev["noisy"][[0, 2, 3, 4], 5] > 0.0)
        with pytest.raises(pkg.BPError, match="status -1"):
            g.eval_mix(plan, 44100, pkg.WAVE_MASK, D, extended="full")
        parity_record(noisy=ev["noisy"].tolist(), enhanced=ev["enhanced"].tolist(), logmmse=lm["enhanced"].tolist(), logmmse_spp=sp["enhanced"].tolist())
    finally:
        g.close()


# ---- 3. bpeval scores=full
def _rows(path):
    return [ln.split() for ln in open(path).read().splitlines()]


def _fmt(a):
    return [["%.9g" % v for v in row] for row in a]


def test_bpeval_scores_full(pkg, tmp_path):
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
    seed, snrs, per, cache = 77, [0.0, 10.0], 2, 3000
    keys = ["clean_list=%s" % (tmp_path / "clean.list"), "noise_list=%s" % (tmp_path / "noise.list"), "norm_file=%s" % (tmp_path / "x.norm"),
            "initwts_file=%s" % (tmp_path / "net.wts"), "fea_dim=%d" % D, "fea_context=%d" % CTX, "targ_offset=%d" % TOFF,
            "layersizes=%s" % ",".join(map(str, ls)), "snr_list=0,10", "mix_per_clean=%d" % per, "init_randem_seed=%d" % seed,
            "traincache=%d" % cache, "bunchsize=32", "baseline=logmmse"]
    r1 = subprocess.run([exe] + keys + ["scores_out=%s" % (tmp_path / "s1.txt"), "scores=extended"], capture_output=True, text=True, timeout=300)
    r2 = subprocess.run([exe] + keys + ["scores_out=%s" % (tmp_path / "s2.txt"), "scores=full"], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 1 and r2.returncode == 1, r1.stdout + r2.stdout + r2.stderr
    # stdout: the extended line up to its SI-SDR figures, then the two new scores, then the undefined count
    l1, l2 = r1.stdout.splitlines(), r2.stdout.splitlines()
    assert len(l1) == len(l2) == 6, r2.stdout
    for ext, full in zip(l1, l2):
        head, tail = full.split(", LLR ")
        assert ext.startswith(head + " (") and "LLR" not in ext and head.count(" -> ") == 5, (ext, full)
        llr, rest = tail.split(", CD ")
        assert len(llr.split(" -> ")) == 2 and rest.split(" dB (")[1].endswith(" undefined)") and len(rest.split(" dB (")[0].split(" -> ")) == 2, full
    # scores_out: the extended rows are what they were (19 fields); the full rows carry them in front of and around the new ones
    rows1, rows2 = _rows(tmp_path / "s1.txt"), _rows(tmp_path / "s2.txt")
    assert all(len(r) == 19 for r in rows1) and all(len(r) == 25 for r in rows2)
    assert [r[:14] for r in rows2] == [r[:14] for r in rows1] and [r[18:23] for r in rows2] == [r[14:] for r in rows1]
    plan = pkg.mix_plan(seed, len(clean), per, [x.size for x in noise], snrs)
    g = pkg.BP_GPU(1, 3, ls, 32, 0.0, 0.0, 0.0, W, b, max_chunk_frames=cache)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps")
        T = g.mix_frames(plan) + CTX - 1                          # bpeval's cut: calls of at most traincache rows
        net, lmm, first, rows_ = [], [], 0, 0
        for i in range(len(plan) + 1):
            if i == len(plan) or rows_ + T[i] > cache:
                ev = g.eval_mix(plan[first:i], FS, extended="full")
                net.append(np.stack([ev["noisy"][:, 5], ev["enhanced"][:, 5], ev["noisy"][:, 6], ev["enhanced"][:, 6]], axis=1))
                lmm.append(g.eval_mix_logmmse(plan[first:i], FS, extended="full")["enhanced"][:, 5:])
                first, rows_ = i, 0
            if i < len(plan):
                rows_ += T[i]
    finally:
        g.close()
    assert [r[14:18] for r in rows2] == _fmt(np.concatenate(net))
    assert [r[23:] for r in rows2] == _fmt(np.concatenate(lmm))
    # pairs mode
    refs = [clean[0], clean[3]]
    ests = [np.round(LP.add_noise(rng, x, 25.0)).clip(-32768, 32767).astype(np.float32) for x in refs]
    lines = []
    for i, (x, y) in enumerate(zip(refs, ests)):
        TE._write_pcm16(tmp_path / ("r%d.wav" % i), x, FS)
        TE._write_pcm16(tmp_path / ("e%d.wav" % i), y, FS)
        lines.append("%s %s\n" % (tmp_path / ("r%d.wav" % i), tmp_path / ("e%d.wav" % i)))
    (tmp_path / "p.list").write_text("".join(lines))
    pk = [exe, "pairs_list=%s" % (tmp_path / "p.list"), "fea_dim=%d" % D]
    p1 = subprocess.run(pk + ["scores_out=%s" % (tmp_path / "p1.txt"), "scores=extended"], capture_output=True, text=True, timeout=300)
    p2 = subprocess.run(pk + ["scores_out=%s" % (tmp_path / "p2.txt"), "scores=full"], capture_output=True, text=True, timeout=300)
    assert p1.returncode == 1 and p2.returncode == 1, p1.stdout + p2.stdout + p2.stderr
    head, tail = p2.stdout.split(", LLR ")
    assert p1.stdout.startswith(head + " (") and ", CD " in tail and tail.endswith(" dB (0 undefined)\n"), (p1.stdout, p2.stdout)
    q1, q2 = _rows(tmp_path / "p1.txt"), _rows(tmp_path / "p2.txt")
    want = pkg.score_waves(0, D, FS, refs, ests, extended="full")
    assert all(len(r) == 7 for r in q1) and q1 == [r[:7] for r in q2] and all(len(r) == 9 for r in q2)     # ref est and the five leading scores
    assert [r[2:] for r in q2] == _fmt(want)
    assert "%.4f" % np.mean(want[:, 5].astype(np.float64)) in tail and "%.3f" % np.mean(want[:, 6].astype(np.float64)) in tail
