"""CPU tests of the critical-band scores fwSegSNR and WSS (no GPU): the float64 restatement in tests/eval_cb_np.py -- its band
table, its fixtures, its precision against 80-bit arithmetic, and the wrong formulas that the GPU bars of
tests/test_eval_cb_gpu.py (1e-4 dB and 1e-4) must catch -- and the argument checks of n_scores = 9, of extended="all" and of
bpeval scores=all that come before any device use.

Mutants: each row of eval_cb_np.MUTANTS must move the restatement by at least 10 bars on the fixture and measure the row names.
Measured (CPU, float64, in bars): gamma 1 11580 (rev8, fwSegSNR); magnitude and power spectra swapped 46390 (rev8, fwSegSNR) and
53880 (rev8, WSS); no normalisation 31990 (rev8, fwSegSNR); no cut of the filters 269 (rev16, WSS; 17 on fwSegSNR there); f0 not
floored 4651, n_fft = 2^ceil(log2 win) 4339, skip = win/2 60, Kmax 1 23980, the true summit B_n 5942, weights from the reference
alone 122 (all rev8, WSS); no window 22940 (rev16, WSS); clamps omitted 86 (rev8, fwSegSNR: one frame of 216 above 35 dB); no
trim on WSS 82980 (burst8); trim on fwSegSNR 3184 (rev8); floor 1e-10 omitted 60940 (faint8, WSS).
The fixtures: fwSegSNR's main pairs stay off its clamps (rev8 0.5 %, every other 0 %); the 30 dB and burst pairs sit 37 .. 60 % on
the upper clamp and are the clamp's fixtures (and main ones for WSS, which has no clamp).  The floor needs band energies below
1e-10, which int16-scaled audio never has: the faint pairs carry noise of 1e-9 where the reference is silent."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import eval_cb_np as CB
import eval_lpc_np as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")
BPEVAL = os.path.join(PKG, "bpeval")
RATES = (8000, 10000, 12000, 16000, 20000, 24000, 32000, 48000, 80000)


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH) or not os.path.exists(BPEVAL):
        import __graft_entry__
        __graft_entry__.build()
    return pkg.load_library()


@pytest.fixture(scope="module")
def fx():
    """eval_cb_np.fixtures(): made once, read only"""
    return CB.fixtures()


@pytest.fixture(scope="module")
def base(fx):
    """{name: (fwSegSNR, WSS)} of the main and clamp fixtures in float64, unrounded: computed once, shared"""
    return {k: CB.scores(r, e, fs, rounded=False) for k, (fs, r, e, kind) in fx.items() if kind != "edge"}


# ---- 1. the band table
def test_band_table_supports_and_margin():
    assert len(CB.CF) == len(CB.BW) == 25
    lo, hi, tot = [], [], []
    for fs in RATES:
        win, _, _ = CB.framing(fs, fs)
        n_fft = CB.fft_size(win)
        assert n_fft // 2 >= win > n_fft // 4 and n_fft <= 8192
        G = CB.band_filters(fs, n_fft // 2)
        cnt = (G > 0).sum(axis=1)
        for i in range(25):                                                         # each support is one run of bins below Nyquist
            k = np.nonzero(G[i])[0]
            assert k.size == cnt[i] > 0 and k[-1] - k[0] + 1 == k.size and k[-1] < n_fft // 2 - 1, (fs, i)
        lo.append(int(cnt.min())); hi.append(int(cnt.max())); tot.append(int(cnt.sum()))
        margin = CB.cut_margin(fs, n_fft // 2)
        print(fs, win, n_fft, lo[-1], hi[-1], tot[-1], margin)
        assert margin >= 1e-6, (fs, margin)                                         # no value a last bit of exp could move across the cut
    assert min(lo) == 7 and max(hi) == 55 and min(tot) == 383 and max(tot) == 619
    assert [CB.fft_size(w) for w in (240, 480, 512, 513, 1440, 2400, 4096)] == [512, 1024, 1024, 2048, 4096, 8192, 8192]


# ---- 2. the fixtures are what the bars are judged on
def test_fixtures_meet_their_conditions(fx, base):
    kinds = {k: v[3] for k, v in fx.items()}
    assert sorted(k for k in kinds if kinds[k] == "main") == sorted(
        [t + s for t in ("rev", "snr5_", "snr15_", "tones", "faint") for s in ("8", "16")] + ["wide48", "wide80"])
    assert sorted(k for k in kinds if kinds[k] == "clamp") == sorted(t + s for t in ("snr30_", "burst") for s in ("8", "16"))
    assert [fx[k][0] for k in ("wide48", "wide80")] == [48000, 80000]
    for name, kind in kinds.items():
        if kind == "edge":
            continue
        fs, r, e, _ = fx[name]
        fw, fv, ws, wv = CB.frame_values(r, e, fs)
        share = CB.clamped_share(r, e, fs)
        print(name, kind, int(fv.sum()), fw.size, share, base[name])
        assert fv.sum() >= 20 and np.array_equal(fv, wv), name
        if kind == "main":
            assert share <= 0.10 and -10.0 < base[name][0] < 35.0, (name, share)
        else:
            assert 0.30 <= share <= 0.65, (name, share)
        assert 0.2 <= base[name][1] <= 25.0, (name, base[name])                     # (the range the WSS bar's rounding term is taken over)
    for tag, fs in (("8", 8000), ("16", 16000)):
        for name in ("rev", "snr15_", "snr5_"):                                     # the speech-like pairs: silent segments, skipped
            _, r, e, _ = fx[name + tag]
            _, fv, _, wv = CB.frame_values(r, e, fs)
            assert fv.size == 262 and fv.sum() == 216 and (~fv).sum() >= 0.10 * fv.size
        # the burst is longer than the trim can drop: more of its frames lie above the 95 % cut than the trim removes
        _, r, e, _ = fx["burst" + tag]
        _, _, ws, wv = CB.frame_values(r, e, fs)
        win, skip, J = CB.framing(r.size, fs)
        a, m = int(0.45 * fs), int((0.10 if fs == 8000 else 0.13) * fs)
        inside = [j for j in range(J) if j * skip + win > a and j * skip < a + m and wv[j]]
        dropped = int(wv.sum()) - LP.keep(int(wv.sum()))
        assert dropped == 11 and len(inside) > dropped, (len(inside), dropped)
        assert np.median(ws[inside]) > 5 * np.median(ws[wv]), tag
        # the faint pairs: every frame valid, band energies below the floor where the reference was silent
        _, r, e, _ = fx["faint" + tag]
        _, fv, ws, wv = CB.frame_values(r, e, fs)
        assert wv.all() and fv.all() and (ws == 0.0).sum() >= 10


def test_properties_and_edges(fx):
    for tag, fs in (("8", 8000), ("16", 16000)):
        _, r, e, _ = fx["same" + tag]
        assert CB.scores(r, e, fs) == (35.0, 0.0)
        got = CB.scores(r, 2 * r, fs)                                               # a gain: fwSegSNR normalises it away, WSS takes slopes
        assert got[0] == 35.0 and abs(got[1]) <= 1e-9, got
        _, r, e, _ = fx["zeros" + tag]
        assert all(math.isnan(v) for v in CB.scores(r, e, fs))
        a, b = CB.scores(*[fx["snr15_" + tag][k] for k in (1, 2, 0)]), CB.scores(*[fx["snr5_" + tag][k] for k in (1, 2, 0)])
        assert a[0] > b[0] and a[1] < b[1], (a, b)                                  # worse with more noise
        for name, J in (("short", 0), ("noframe", 0), ("oneframe", 1), ("jv10_", 10), ("jv11_", 11)):
            f, r, e, _ = fx[name + tag]
            fw, fv, ws, wv = CB.frame_values(r, e, f)
            assert fv.size == J and fv.sum() == J and wv.sum() == J, (name, tag)
            got = CB.scores(r, e, f)
            assert all(math.isnan(v) for v in got) if J == 0 else all(math.isfinite(v) for v in got), (name, tag, got)
        f, r, e, _ = fx["lead" + tag]                                               # the exact-zero lead: its frames are skipped
        _, fv, _, wv = CB.frame_values(r, e, f)
        win, skip, _ = CB.framing(r.size, f)
        lead = int(0.1 * fs)
        assert not wv[:(lead - win) // skip + 1].any() and wv[lead // skip + 1] and np.array_equal(fv, wv)


def test_nearest_peak_search():
    B = np.array([[0.0, 1.0, 3.0, 2.0, 2.0, 1.0, 4.0, 5.0] + [5.0 - k for k in range(1, 18)]])
    L = CB.nearest_peak(B)[0]
    # rising at 0, 1: the summit is band 2, the band below it band 1; falling (or level) at 2 .. 4: back to the summit, band 2;
    # rising at 5, 6: summit band 7, below it band 6; falling from 7 on: band 7
    assert L[:8].tolist() == [1.0, 1.0, 3.0, 3.0, 3.0, 4.0, 4.0, 5.0] and np.all(L[8:] == 5.0)
    assert CB.nearest_peak(B, true_summit=True)[0][:7].tolist() == [3.0, 3.0, 3.0, 3.0, 3.0, 5.0, 5.0]
    up = np.arange(25.0)[None, :]                                                   # rising to the end: n stops at 24
    assert np.all(CB.nearest_peak(up)[0] == 23.0)
    assert np.all(CB.nearest_peak(-up)[0] == 0.0)                                   # falling from the start: n runs to -1


# ---- 3. float64 is enough
def test_float64_against_longdouble(fx, base):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no wider long double on this machine")
    worst = [0.0, 0.0]
    for name in base:
        fs, r, e, _ = fx[name]
        _, _, J = CB.framing(r.size, fs)
        sub = np.arange(0, J, 16 if fs <= 16000 else 12)                            # (a direct DFT: a subset of the frames)
        a, b = CB.frame_values(r, e, fs, frames=sub), CB.frame_values(r, e, fs, np.longdouble, frames=sub)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        worst = [max(worst[0], float(np.abs(a[0] - b[0]).max())), max(worst[1], float(np.abs(a[2] - b[2]).max()))]
    print(worst)
    assert worst[0] <= 1e-6 and worst[1] <= 1e-6, worst


# ---- 4. the bars catch a wrong formula
@pytest.mark.parametrize("name", sorted(CB.MUTANTS))
def test_bar_catches_mutant(fx, base, name):
    kw, where, measure = CB.MUTANTS[name]
    fs, r, e, kind = fx[where]
    assert kind == "main" or (measure == "wss" and kind == "clamp")
    k, bar = (0, CB.BAR_FW) if measure == "fw" else (1, CB.BAR_WSS)
    shift = float(abs(CB.scores(r, e, fs, rounded=False, **kw)[k] - base[where][k]))
    print(name, where, measure, "%.3g = %.3g bars" % (shift, shift / bar))
    assert shift >= 10 * bar, (name, shift)


# ---- 5. argument errors before any device use
def _score_ext(lib, n_scores, fs=8000, fea_dim=129, est=True):
    lens = np.array([100], np.int32)
    r, e, o = np.zeros(100, np.float32), np.zeros(100, np.float32), np.zeros((1, 16), np.float32)
    fp = C.POINTER(C.c_float)
    return lib.bp_score_waves_ext(0, fea_dim, fs, 1, lens.ctypes.data_as(C.POINTER(C.c_int)), r.ctypes.data_as(fp),
                                  e.ctypes.data_as(fp) if est else None, n_scores, o.ctypes.data_as(fp))


def test_n_scores_9_is_accepted_as_far_as_the_next_check(lib, pkg):
    assert pkg.SCORE_ALL_N == 9
    # 9 passes the n_scores check: the next checks of bp_score_waves answer, in its order
    assert _score_ext(lib, 9, fs=44100) == -1 and b"sample_rate" in lib.bp_last_error() and b"n_scores" not in lib.bp_last_error()
    assert _score_ext(lib, 9, fea_dim=100) == -1 and b"power of two" in lib.bp_last_error()
    for ns in (8, 10, 11, 4, 0, 6, -3, 2):
        assert _score_ext(lib, ns) == -1 and b"bp_score_waves_ext: n_scores must be" in lib.bp_last_error(), ns
    # the two checks of nine columns: all 25 bands below Nyquist, n_fft <= 8192; in the caller's name, and not with seven
    assert _score_ext(lib, 9, fs=5000) == -1 and b"bp_score_waves_ext: sample_rate must be at least 8000" in lib.bp_last_error()
    assert _score_ext(lib, 9, fs=160000) == -1 and b"bp_score_waves_ext: sample_rate" in lib.bp_last_error() and b"4096" in lib.bp_last_error()
    for fs in (5000, 160000):                                                       # (7: the rate passes, the next check answers)
        assert _score_ext(lib, 7, fs=fs, est=False) == -1 and b"null pointer" in lib.bp_last_error() and b"sample_rate" not in lib.bp_last_error()
        assert _score_ext(lib, 9, fs=fs, est=False) == -1 and b"sample_rate" in lib.bp_last_error()
    m = np.zeros(1, pkg.MIXTURE_DTYPE)
    s = np.zeros((1, 9), np.float32)
    fp = C.POINTER(C.c_float)
    mp, sp = m.ctypes.data_as(C.c_void_p), s.ctypes.data_as(fp)
    assert lib.bp_eval_mix_ext(None, 1, mp, 8000, 0, 0, 9, sp, sp, None) == -1 and b"null handle" in lib.bp_last_error()
    assert lib.bp_eval_mix_ext(None, 1, mp, 8000, 0, 0, 8, sp, sp, None) == -1 and b"bp_eval_mix_ext: n_scores" in lib.bp_last_error()
    assert lib.bp_eval_mix_logmmse_ext(None, None, 1, mp, 8000, 9, sp, sp, None) == -1 and b"n_scores" not in lib.bp_last_error()
    assert lib.bp_eval_mix_logmmse_ext(None, None, 1, mp, 8000, 10, sp, sp, None) == -1 and b"bp_eval_mix_logmmse_ext: n_scores" in lib.bp_last_error()
    assert lib.bp_eval_mix_logmmse_nt(None, None, None, 1, mp, 8000, 9, sp, sp, None) == -1 and b"n_scores" not in lib.bp_last_error()
    assert lib.bp_eval_mix_logmmse_nt(None, None, None, 1, mp, 8000, 11, sp, sp, None) == -1 and b"bp_eval_mix_logmmse_nt: n_scores" in lib.bp_last_error()


def test_constants_header_and_kernels(lib, pkg):
    assert (pkg.SCORE_FWSSNR, pkg.SCORE_WSS, pkg.SCORE_ALL_N) == (7, 8, 9)
    hdr = open(os.path.join(ROOT, "include", "bp_c_api.h")).read()
    assert "enum { BP_SCORE_FWSSNR = 7, BP_SCORE_WSS = 8, BP_SCORE_ALL_N = 9 };" in hdr
    assert lib.bp_abi_version() == 5
    data = open(pkg.LIB_PATH, "rb").read()
    for k in ("bp_eval_cb", "bp_eval_cbsum", "bp_eval_lpcrank"):
        assert re.search(rb"_Z\d+" + k.encode() + rb"N\w*\.kd", data), k


def test_extended_takes_all(pkg, monkeypatch):
    assert pkg._abi.score_columns("x", "all") == 9 and pkg._abi.score_columns("x", "full") == 7
    r = [np.zeros(100, np.float32)]
    called = []
    monkeypatch.setattr(pkg.signal, "load_library", lambda *a: called.append(1))
    for bad in ("Full", "extended", 7, 5, 1, 0, None, "", 2.0, "All", "ALL", "all ", 9):
        with pytest.raises(pkg.BPError, match="extended must be False, True or \"full\", or \"all\" for the nine columns"):
            pkg.score_waves(0, 129, 8000, r, r, extended=bad)
        for call in (pkg.BP_GPU.eval_mix, pkg.BP_GPU.eval_mix_logmmse):
            with pytest.raises(pkg.BPError, match="extended must be"):
                call(None, None, 8000, extended=bad)                                 # (before the handle or the plan is looked at)
        with pytest.raises(pkg.BPError, match="extended must be"):
            pkg.BP_GPU.eval_mix_logmmse(None, None, 8000, extended=bad, noise="spp")
    assert not called
    # "all" passes that check: the call goes on to the handle it was not given
    for kw in ({}, {"noise": "spp"}):
        with pytest.raises(Exception) as ei:
            pkg.BP_GPU.eval_mix_logmmse(None, None, 8000, extended="all", **kw)
        assert "extended must be" not in str(ei.value)
    with pytest.raises(Exception) as ei:
        pkg.BP_GPU.eval_mix(None, None, 8000, extended="all")
    assert "extended must be" not in str(ei.value)


def _bpeval(*args):
    r = subprocess.run([BPEVAL] + list(args), capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r                 # (errors: exit(0); success returns 1)
    return r.stdout


def test_bpeval_takes_scores_all(lib, tmp_path):
    (tmp_path / "none.pairs").write_text("")
    for bad in ("Full", "FULL", "full ", "extended|full", "7", "bogus", "", "Extended", "basic|extended", "All", "ALL", "all ", "full|all", "9"):
        assert _bpeval("pairs_list=%s" % (tmp_path / "none.pairs"), "fea_dim=129", "scores=" + bad) == "bpeval: bad value for scores: %s\n" % bad
    # all is a key of both modes: the run goes on to its next check, with and without the baseline
    assert "can not open pairs_list" in _bpeval("pairs_list=%s" % (tmp_path / "nope.pairs"), "fea_dim=129", "scores=all")
    assert "need norm_file and initwts_file" in _bpeval("fea_dim=129", "fea_context=3", "layersizes=387,64,129", "scores=all")
    assert "need norm_file and initwts_file" in _bpeval("fea_dim=129", "fea_context=3", "layersizes=387,64,129", "scores=all", "baseline=logmmse")
