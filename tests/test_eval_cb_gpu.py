"""GPU tests of the critical-band scores fwSegSNR and WSS (the _ext calls with nine columns, extended="all"; -m gpu) against the
float64 restatement in tests/eval_cb_np.py and against the calls they are made of.

Bars, absolute: fwSegSNR 1e-4 dB, WSS 1e-4.  The arithmetic is double against double and the result is rounded once to fp32: half
an ulp is 1.9e-6 at 35 dB and 7.6e-6 below 128 (the main pairs' WSS lies in 0.2 .. 25: tests/test_eval_cb_host.py), and float64
against 80-bit arithmetic differs by at most 5.2e-12 per frame on these fixtures (there, against a bar of 1e-6): both bars leave
more than 10 x over that.  The NaN pattern must be equal.  tests/test_eval_cb_host.py shows that these bars catch a wrong formula.
Everything else is bit for bit: the same bits on every run, in any order and in any company, columns 0..6 the seven-column call,
the narrower calls untouched by a nine-column call before them on the same handle, and the eval_mix calls equal to score_waves
on their own audio."""
import functools

import numpy as np
import pytest

import eval_cb_np as CB
import test_eval_gpu as TE

pytestmark = pytest.mark.gpu
FS, D, CTX, TOFF = TE.FS, TE.D, TE.CTX, TE.TOFF
_bits = TE._bits
FEA = {8000: 129, 16000: 257, 48000: 257, 80000: 257}


@functools.lru_cache(maxsize=None)
def _set(fs):
    """(names, refs, ests, want [n][2]) of eval_cb_np.fixtures() at fs, the restatement's scores beside them: made once, read only"""
    fx = {k: v for k, v in _fixtures().items() if v[0] == fs}
    names = sorted(fx)
    refs, ests = [fx[k][1] for k in names], [fx[k][2] for k in names]
    want = np.array([CB.scores(r, e, fs) for r, e in zip(refs, ests)], np.float64)
    return names, refs, ests, want


@functools.lru_cache(maxsize=None)
def _fixtures():
    return CB.fixtures()


# ---- (a) against the restatement, all fixtures of a rate in one call
@pytest.mark.parametrize("fs", [8000, 16000, 48000, 80000])
def test_score_waves_all_match_restatement(pkg, fs, parity_record):
    names, refs, ests, want = _set(fs)
    got = pkg.score_waves(0, FEA[fs], fs, refs, ests, extended="all")
    assert got.shape == (len(refs), 9) and got.dtype == np.float32
    fw, ws = got[:, pkg.SCORE_FWSSNR].astype(np.float64), got[:, pkg.SCORE_WSS].astype(np.float64)
    nan = np.isnan(want)
    diff = np.abs(np.stack([fw, ws], axis=1) - want)
    err = {"fwssnr_db": float(np.nanmax(diff[:, 0])), "wss_abs": float(np.nanmax(diff[:, 1]))}
    print(fs, err)
    for k, name in enumerate(names):
        print("  %-11s fwSegSNR %.6f (%.6f)  WSS %.6f (%.6f)" % (name, fw[k], want[k, 0], ws[k], want[k, 1]))
    parity_record(fs=fs, names=names, fwssnr=fw.tolist(), wss=ws.tolist(), diff_fwssnr=diff[:, 0].tolist(), diff_wss=diff[:, 1].tolist(),
                  bar_fwssnr_db=CB.BAR_FW, bar_wss=CB.BAR_WSS, **err)
    assert np.array_equal(np.isnan(fw), nan[:, 0]) and np.array_equal(np.isnan(ws), nan[:, 1]), (names, got[:, 7:])
    if fs <= 16000:
        assert nan[:, 0].sum() == 3 and (~nan[:, 0]).sum() == 12                   # zeros, short, noframe; everything else is scored
    else:
        assert len(names) == 1 and not nan.any()
    assert err["fwssnr_db"] <= CB.BAR_FW and err["wss_abs"] <= CB.BAR_WSS, err
    # columns 0..6: the seven-column call
    assert np.array_equal(_bits(got[:, :7]), _bits(pkg.score_waves(0, FEA[fs], fs, refs, ests, extended="full")))


# ---- (b) the same bits on every run, in any order, alone
@pytest.mark.parametrize("fs", [8000, 16000])
def test_all_columns_order_and_company(pkg, fs):
    names, refs, ests, _ = _set(fs)
    D_ = FEA[fs]
    nine = pkg.score_waves(0, D_, fs, refs, ests, extended="all")
    assert np.array_equal(_bits(nine), _bits(pkg.score_waves(0, D_, fs, refs, ests, extended="all")))         # two calls, the same bits
    back = pkg.score_waves(0, D_, fs, refs[::-1], ests[::-1], extended="all")
    assert np.array_equal(_bits(back[::-1]), _bits(nine))                                                   # reversed order
    tag = "8" if fs == 8000 else "16"
    for name in ("burst" + tag, "faint" + tag, "oneframe" + tag, "zeros" + tag, "noframe" + tag):          # a pair alone
        k = names.index(name)
        alone = pkg.score_waves(0, D_, fs, [refs[k]], [ests[k]], extended="all")
        assert np.array_equal(_bits(alone[0]), _bits(nine[k])), name
    # the narrower calls after a nine-column call are what the nine-column call holds
    assert np.array_equal(_bits(pkg.score_waves(0, D_, fs, refs, ests, extended=True)), _bits(nine[:, :5]))
    assert np.array_equal(_bits(pkg.score_waves(0, D_, fs, refs, ests)), _bits(nine[:, :3]))


# ---- (c) the mix calls
def test_eval_mix_all_is_score_waves_on_its_own_audio(pkg, parity_record):
    rng = np.random.default_rng(11)
    clean, noise = TE._corpus(rng)
    mean, istd = TE._norm(rng)
    plan = TE._plan(pkg)
    g = TE._handle(pkg, False, False)
    try:
        g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps+irm")
        seven = g.eval_mix(plan, FS, pkg.WAVE_MASK, D, extended="full")
        seven_lm = g.eval_mix_logmmse(plan, FS, extended="full")
        ev = g.eval_mix(plan, FS, pkg.WAVE_MASK, D, return_pcm=True, extended="all")
        lm = g.eval_mix_logmmse(plan, FS, return_pcm=True, extended="all")
        sp = g.eval_mix_logmmse(plan, FS, return_pcm=True, extended="all", noise="spp")
        lens = [clean[c].size for c in plan["clean"]]
        mix = np.split(g.mix_features(plan)["pcm"], np.cumsum(lens)[:-1])
        refs = [clean[c] for c in plan["clean"]]
        noisy = pkg.score_waves(0, D, FS, refs, mix, extended="all")
        for out in (ev, lm, sp):
            assert out["noisy"].shape == out["enhanced"].shape == (len(plan), 9)
            assert np.array_equal(_bits(out["noisy"]), _bits(noisy))
            assert np.array_equal(_bits(out["enhanced"]), _bits(pkg.score_waves(0, D, FS, refs, out["pcm"], extended="all")))
        assert not np.array_equal(_bits(lm["enhanced"][:, 7:]), _bits(sp["enhanced"][:, 7:]))
        # columns 0..6, and the seven-column call after the nine-column ones
        again = g.eval_mix(plan, FS, pkg.WAVE_MASK, D, extended="full")
        for k in ("noisy", "enhanced"):
            assert np.array_equal(_bits(ev[k][:, :7]), _bits(seven[k])) and np.array_equal(_bits(again[k]), _bits(seven[k]))
            assert np.array_equal(_bits(lm[k][:, :7]), _bits(seven_lm[k]))
        # mixture 1 has a silent noise: x == s
        assert ev["noisy"][1, pkg.SCORE_FWSSNR] == 35.0 and ev["noisy"][1, pkg.SCORE_WSS] == 0.0, ev["noisy"][1]
        assert np.all(np.isfinite(ev["noisy"][:, 7:])) and np.all(ev["noisy"][[0, 2, 3, 4], 8] > 0.0)
        with pytest.raises(pkg.BPError, match="status -1"):
            g.eval_mix(plan, 5000, pkg.WAVE_MASK, D, extended="all")
        parity_record(noisy=ev["noisy"].tolist(), enhanced=ev["enhanced"].tolist(), logmmse=lm["enhanced"].tolist(), logmmse_spp=sp["enhanced"].tolist())
    finally:
        g.close()


# ---- (d) the work buffers a nine-column call leaves behind
def test_narrower_calls_after_a_dyed_nine_column_call(pkg):
    rng = np.random.default_rng(12)
    clean, noise = TE._corpus(rng)
    clean = clean + [np.full(40000, np.nan, np.float32)]                            # entry 4: NaN into every buffer that reads it
    mean, istd = TE._norm(rng)
    plan = TE._plan(pkg)
    big = np.zeros(3, pkg.MIXTURE_DTYPE)
    for i, m in enumerate([(4, 2, 0, 0.0), (2, 2, 100, 5.0), (4, 0, 0, 10.0)]):
        big[i] = m
    widths = (False, True, "full")
    fresh, used = TE._handle(pkg, False, False), TE._handle(pkg, False, False)
    try:
        for g in (fresh, used):
            g.set_mix_corpus(clean, noise, mean, istd, CTX, TOFF, "lps+irm")
        dyed = used.eval_mix(big, FS, pkg.WAVE_MASK, D, extended="all")
        assert dyed["noisy"].shape == (3, 9) and np.isnan(dyed["noisy"][[0, 2]]).any(axis=1).all() and np.all(np.isfinite(dyed["noisy"][1]))
        used.eval_mix_logmmse(big, FS, extended="all")
        for ext in widths:
            a, b = fresh.eval_mix(plan, FS, pkg.WAVE_MASK, D, extended=ext), used.eval_mix(plan, FS, pkg.WAVE_MASK, D, extended=ext)
            la, lb = fresh.eval_mix_logmmse(plan, FS, extended=ext), used.eval_mix_logmmse(plan, FS, extended=ext)
            for k in ("noisy", "enhanced"):
                assert np.array_equal(_bits(a[k]), _bits(b[k])) and np.array_equal(_bits(la[k]), _bits(lb[k])), (ext, k)
    finally:
        fresh.close()
        used.close()
