"""CPU tests of the spectral-envelope scores LLR and cepstral distance (no GPU): the float64 restatement in tests/eval_lpc_np.py
-- its fixtures, its edge lengths, its precision against 80-bit arithmetic, and the wrong formulas that the GPU bars of
tests/test_eval_lpc_gpu.py (LLR 1e-5, CD 1e-4 dB) must catch -- and the argument checks of n_scores = 7, of extended="full" and
of bpeval scores=full that come before any device use.

Mutants: each row of eval_lpc_np.MUTANTS must move the restatement by at least 10 bars on the main fixture and measure the row
names.  Measured (CPU, float64, in bars): P + 1 765 and P - 1 560 (rev8, CD); no window 695 (rev16, LLR); no trim 725 (rev8,
LLR); no clamp 931 (burst8, LLR); correction omitted 842 (tones16, LLR) -- on the reverberant and 30 dB pairs it moves the scores
by 1 .. 6 bars only, which is why the tone pairs are main fixtures; correction 1e-4 87 (rev16, LLR); A_e and A_r swapped and T
from R_e 4991 (rev8, LLR: both send every frame to the lower clamp); cepstrum without q/m 10533 (rev8, CD); ties not broken (every
equal frame counts against a frame) 6590 (burst8, LLR).  The no-clamp and the tie rows need more frames on the upper clamp than
the trim drops (5 %), and the main fixtures at most 10 %: the burst pairs (8.3 % and 9.7 %) are there for that.
Ties broken the other way (the higher index first) selects other frames on the burst pairs but exchanges equal values only: it
moves no score, on no signal, and no bar can catch it; test_reversed_tie_order_moves_the_frames_but_no_score holds that."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import eval_lpc_np as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")
BPEVAL = os.path.join(PKG, "bpeval")


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH) or not os.path.exists(BPEVAL):
        import __graft_entry__
        __graft_entry__.build()
    return pkg.load_library()


@pytest.fixture(scope="module")
def fx():
    """eval_lpc_np.fixtures(): made once, read only"""
    return LP.fixtures()


@pytest.fixture(scope="module")
def base(fx):
    """{name: (LLR, CD)} of the main fixtures in float64, unrounded: computed once, shared by the precision and mutant tests"""
    return {k: LP.llr_cd(r, e, fs, rounded=False) for k, (fs, r, e, kind) in fx.items() if kind == "main"}


# ---- 1. the fixtures are what the bars are judged on
def test_main_fixtures_have_frames_and_stay_off_the_clamps(fx, base):
    assert sorted(base) == sorted(t + s for t in ("rev", "snr30_", "burst", "tones") for s in ("8", "16"))
    for name in base:
        fs, r, e, _ = fx[name]
        _, _, valid = LP.frame_values(r, e, fs)
        share = LP.clamped_share(r, e, fs)
        print(name, int(valid.sum()), share, base[name])
        assert valid.sum() >= 20, name
        assert max(share) <= 0.10, (name, share)
        assert 0.0 < base[name][0] < 2.0 and 0.0 < base[name][1] < 10.0, (name, base[name])
    # the speech-like pairs hold silent segments (invalid frames); the 5 dB pair is there for the clamps
    for tag in ("8", "16"):
        fs, r, e, _ = fx["rev" + tag]
        _, _, valid = LP.frame_values(r, e, fs)
        assert 0 < valid.sum() < valid.size
        fs, r, e, _ = fx["snr5_" + tag]
        assert max(LP.clamped_share(r, e, fs)) > 0.10


def test_properties(fx):
    for tag in ("8", "16"):
        fs, r, e, _ = fx["same" + tag]
        assert LP.llr_cd(r, e, fs) == (0.0, 0.0)
        assert LP.llr_cd(r, 2 * r, fs) == pytest.approx((0.0, 0.0), abs=1e-9)       # (a gain changes neither envelope measure)
        fs, r, e, _ = fx["zeros" + tag]
        assert all(math.isnan(v) for v in LP.llr_cd(r, e, fs))
        a, b = LP.llr_cd(*[fx["snr30_" + tag][k] for k in (1, 2, 0)]), LP.llr_cd(*[fx["snr5_" + tag][k] for k in (1, 2, 0)])
        assert a[0] < b[0] and a[1] < b[1], (a, b)                                   # worse with more noise


# ---- 2. edge lengths
def test_edge_lengths(fx):
    assert [LP.keep(j) for j in (1, 10, 11, 20, 216)] == [1, 10, 10, 19, 205]
    for tag, fs in (("8", 8000), ("16", 16000)):
        win, skip, _ = LP.framing(fs, fs)
        for name, n, J in (("short", win - 1, 0), ("noframe", win + skip - 1, 0), ("oneframe", win + skip, 1), ("jv10_", win + 10 * skip, 10),
                           ("jv11_", win + 11 * skip, 11)):
            f, r, e, _ = fx[name + tag]
            llr, cd, valid = LP.frame_values(r, e, f)
            assert r.size == n and valid.size == J and valid.sum() == J, (name, tag)
            got = LP.llr_cd(r, e, f)
            assert all(math.isnan(v) for v in got) if J == 0 else all(math.isfinite(v) for v in got), (name, tag, got)
            if J:
                assert LP.selected(llr, valid).size == LP.keep(J) == (10 if J == 11 else J)
        f, r, e, _ = fx["lead" + tag]                                               # the exact-zero lead: its frames are skipped
        llr, cd, valid = LP.frame_values(r, e, f)
        lead = int(0.1 * fs)
        assert not valid[:(lead - win) // skip + 1].any() and valid[lead // skip + 1]
        assert all(math.isfinite(v) for v in LP.llr_cd(r, e, f))


# ---- 3. float64 is enough
def test_float64_against_longdouble(fx, base):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("no wider long double on this machine")
    worst = [0.0, 0.0]
    for name, b in base.items():
        fs, r, e, _ = fx[name]
        w = LP.llr_cd(r, e, fs, dt=np.longdouble, rounded=False)
        worst = [max(worst[k], float(abs(w[k] - b[k]))) for k in (0, 1)]
    print(worst)
    assert worst[0] <= 1e-8 and worst[1] <= 1e-8, worst


# ---- 4. the bars catch a wrong formula
@pytest.mark.parametrize("name", sorted(LP.MUTANTS))
def test_bar_catches_mutant(fx, base, name):
    kw, where, measure = LP.MUTANTS[name]
    fs, r, e, kind = fx[where]
    assert kind == "main"
    k, bar = (0, LP.BAR_LLR) if measure == "llr" else (1, LP.BAR_CD)
    shift = float(abs(LP.llr_cd(r, e, fs, rounded=False, **kw)[k] - base[where][k]))
    print(name, where, measure, "%.3g = %.3g bars" % (shift, shift / bar))
    assert shift >= 10 * bar, (name, shift)


def test_reversed_tie_order_moves_the_frames_but_no_score(fx, base):
    moved = 0
    for name in base:
        fs, r, e, _ = fx[name]
        llr, cd, valid = LP.frame_values(r, e, fs)
        for v in (llr, cd):
            a, b = LP.selected(v, valid), LP.selected(v, valid, ties="high_index_first")
            moved += not np.array_equal(a, b)
            assert a.size == b.size and np.array_equal(np.sort(v[a]), np.sort(v[b])), name      # the same values, frame for frame
    assert moved >= 2                                                                           # (the burst pairs: ties across the cut)


# ---- 5. argument errors before any device use
def _score_ext(lib, n_scores, fs=8000, fea_dim=129):
    lens = np.array([100], np.int32)
    r, e, o = np.zeros(100, np.float32), np.zeros(100, np.float32), np.zeros((1, 8), np.float32)
    fp = C.POINTER(C.c_float)
    return lib.bp_score_waves_ext(0, fea_dim, fs, 1, lens.ctypes.data_as(C.POINTER(C.c_int)), r.ctypes.data_as(fp), e.ctypes.data_as(fp),
                                  n_scores, o.ctypes.data_as(fp))


def test_n_scores_7_is_accepted_as_far_as_the_next_check(lib, pkg):
    assert pkg.SCORE_FULL_N == 7
    # 7 passes the n_scores check: the next checks of bp_score_waves answer, in its order
    assert _score_ext(lib, 7, fs=44100) == -1 and b"sample_rate" in lib.bp_last_error() and b"n_scores" not in lib.bp_last_error()
    assert _score_ext(lib, 7, fea_dim=100) == -1 and b"power of two" in lib.bp_last_error()
    for ns in (4, 0, 6, -3, 2, 8):
        assert _score_ext(lib, ns) == -1 and b"bp_score_waves_ext: n_scores must be" in lib.bp_last_error(), ns
    m = np.zeros(1, pkg.MIXTURE_DTYPE)
    s = np.zeros((1, 7), np.float32)
    fp = C.POINTER(C.c_float)
    mp, sp = m.ctypes.data_as(C.c_void_p), s.ctypes.data_as(fp)
    assert lib.bp_eval_mix_ext(None, 1, mp, 8000, 0, 0, 7, sp, sp, None) == -1 and b"null handle" in lib.bp_last_error()
    assert lib.bp_eval_mix_ext(None, 1, mp, 8000, 0, 0, 6, sp, sp, None) == -1 and b"bp_eval_mix_ext: n_scores" in lib.bp_last_error()
    assert lib.bp_eval_mix_logmmse_ext(None, None, 1, mp, 8000, 7, sp, sp, None) == -1 and b"n_scores" not in lib.bp_last_error()
    assert lib.bp_eval_mix_logmmse_ext(None, None, 1, mp, 8000, 6, sp, sp, None) == -1 and b"bp_eval_mix_logmmse_ext: n_scores" in lib.bp_last_error()
    assert lib.bp_eval_mix_logmmse_nt(None, None, None, 1, mp, 8000, 7, sp, sp, None) == -1 and b"n_scores" not in lib.bp_last_error()
    assert lib.bp_eval_mix_logmmse_nt(None, None, None, 1, mp, 8000, 6, sp, sp, None) == -1 and b"bp_eval_mix_logmmse_nt: n_scores" in lib.bp_last_error()


def test_constants_header_and_kernels(lib, pkg):
    import re
    assert (pkg.SCORE_LLR, pkg.SCORE_CD, pkg.SCORE_FULL_N) == (5, 6, 7)
    hdr = open(os.path.join(ROOT, "include", "bp_c_api.h")).read()
    assert "enum { BP_SCORE_LLR = 5, BP_SCORE_CD = 6, BP_SCORE_FULL_N = 7 };" in hdr
    assert lib.bp_abi_version() == 5
    data = open(pkg.LIB_PATH, "rb").read()
    for k in ("bp_eval_lpc", "bp_eval_lpcrank", "bp_eval_lpcsum"):
        assert re.search(rb"_Z\d+" + k.encode() + rb"\w*\.kd", data), k


def test_extended_takes_false_true_and_full_only(pkg, monkeypatch):
    r = [np.zeros(100, np.float32)]
    called = []
    monkeypatch.setattr(pkg.signal, "load_library", lambda *a: called.append(1))
    for bad in ("Full", "extended", 7, 5, 1, 0, None, "", 2.0):
        with pytest.raises(pkg.BPError, match="extended must be False, True or \"full\""):
            pkg.score_waves(0, 129, 8000, r, r, extended=bad)
        for call in (pkg.BP_GPU.eval_mix, pkg.BP_GPU.eval_mix_logmmse):
            with pytest.raises(pkg.BPError, match="extended must be"):
                call(None, None, 8000, extended=bad)                                 # (before the handle or the plan is looked at)
        with pytest.raises(pkg.BPError, match="extended must be"):
            pkg.BP_GPU.eval_mix_logmmse(None, None, 8000, extended=bad, noise="spp")
    assert not called


def _bpeval(*args):
    r = subprocess.run([BPEVAL] + list(args), capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r                 # (errors: exit(0); success returns 1)
    return r.stdout


def test_bpeval_takes_scores_full(lib, tmp_path):
    (tmp_path / "none.pairs").write_text("")
    for bad in ("Full", "FULL", "full ", "extended|full", "7"):
        assert _bpeval("pairs_list=%s" % (tmp_path / "none.pairs"), "fea_dim=129", "scores=" + bad) == "bpeval: bad value for scores: %s\n" % bad
    # full is a key of both modes: the run goes on to its next check, with and without the baseline
    assert "can not open pairs_list" in _bpeval("pairs_list=%s" % (tmp_path / "nope.pairs"), "fea_dim=129", "scores=full")
    assert "need norm_file and initwts_file" in _bpeval("fea_dim=129", "fea_context=3", "layersizes=387,64,129", "scores=full")
    assert "need norm_file and initwts_file" in _bpeval("fea_dim=129", "fea_context=3", "layersizes=387,64,129", "scores=full", "baseline=logmmse")
