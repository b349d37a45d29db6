"""CPU tests of the extended scores (no GPU): the float64 restatement of ESTOI and SI-SDR in tests/eval_ext_np.py -- tied to
tests/eval_np.py through STOI, its properties, and the wrong formulas that the GPU bars of tests/test_eval_ext_gpu.py (ESTOI 1e-4,
SI-SDR 1e-4 dB) must catch -- and the argument checks of bpeval scores= and of n_scores that come before any device use.

Mutants: each wrong formula must move the restatement by at least 10 bars on at least one pair of eval_ext_np.pair_set at 8 or
16 kHz.  Measured maxima over those pairs (CPU, float64): ESTOI without the row step 0.52, without the column step 0.25, with STOI's
scale-and-clip in front 0.013; SI-SDR with alpha = 1 3.0 dB (the scaled pair; 0.0004 .. 0.08 dB on the unscaled ones); SI-SDR with
the means removed 7.4e-4 dB on the pairs without an offset -- white noise and speech_like have next to no mean, so that those pairs
alone do not reach 10 bars -- and 0.085 dB on the pair with an offset of 100, which is in the set for that reason."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import eval_ext_np as EX
import eval_np as EN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")
BPEVAL = os.path.join(PKG, "bpeval")
BAR_ESTOI, BAR_SISDR = 1e-4, 1e-4             # the GPU bars


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH) or not os.path.exists(BPEVAL):
        import __graft_entry__
        __graft_entry__.build()
    return pkg.load_library()


@pytest.fixture(scope="module")
def sets():
    """{fs: (refs, ests)}: made once, read only."""
    return {fs: EX.pair_set(np.random.default_rng(fs), fs) for fs in (8000, 16000)}


def _pairs(sets):
    for fs, (refs, ests) in sets.items():
        for r, e in zip(refs, ests):
            yield fs, r, e


# ---- 1. the two files agree
def test_restated_front_end_reproduces_stoi(sets):
    for fs, r, e in _pairs(sets):
        assert EX.stoi_from_front(r, e, fs, check_margin=True) == EN.stoi(r, e, fs, check_margin=True), fs
    short = EN.speech_like(np.random.default_rng(1), 2400, 8000, gaps=0)
    assert math.isnan(EX.stoi_from_front(short, short, 8000)) and math.isnan(EN.stoi(short, short, 8000))


# ---- 2. properties
def test_estoi_identity_scale_zero():
    rng = np.random.default_rng(3)
    for fs in (8000, 16000):
        r = EN.speech_like(rng, 3 * fs, fs)
        assert abs(EX.estoi(r, r, fs, check_margin=True) - 1.0) < 1e-9
        assert abs(EX.estoi(r, 3 * r, fs) - 1.0) < 1e-9
        assert EX.estoi(r, np.zeros_like(r), fs) == 0.0


def test_scores_rise_with_the_snr():
    rng = np.random.default_rng(4)
    r = EN.speech_like(rng, 3 * 16000, 16000)
    es = [EN.add_noise(rng, r, snr) for snr in (0.0, 10.0, 20.0)]
    a = [EX.estoi(r, e, 16000) for e in es]
    b = [EX.sisdr(r, e) for e in es]
    assert a[0] < a[1] < a[2], a
    assert b[0] < b[1] < b[2], b
    assert [abs(x - snr) < 0.2 for x, snr in zip(b, (0.0, 10.0, 20.0))] == [True] * 3, b   # (white noise: SI-SDR is about the SNR)


def test_sisdr_scale_zero_and_silence():
    rng = np.random.default_rng(5)
    r = EN.speech_like(rng, 20000, 8000)
    e = EN.add_noise(rng, r, 7.0).astype(np.float64)
    assert abs(EX.sisdr(r, 0.5 * e) - EX.sisdr(r, e)) < 1e-9
    assert EX.sisdr(r, np.zeros_like(r)) == 10 * math.log10(EX.EPS)
    z = np.zeros(20000, np.float32)
    assert math.isnan(EX.sisdr(z, e)) and math.isnan(EX.estoi(z, e, 8000))
    s5 = EX.scores5(r, e, 8000, 129)
    assert s5.shape == (5,) and np.array_equal(s5[:3], EN.scores(r, e, 8000, 129))
    assert s5[3] == EX.estoi(r, e, 8000) and s5[4] == EX.sisdr(r, e)


# ---- 3. the bars catch a wrong formula
MUTANTS = [("estoi", dict(rows=False), BAR_ESTOI), ("estoi", dict(cols=False), BAR_ESTOI), ("estoi", dict(clip=True), BAR_ESTOI),
           ("sisdr", dict(unit_alpha=True), BAR_SISDR), ("sisdr", dict(remove_mean=True), BAR_SISDR)]


@pytest.mark.parametrize("which,kw,bar", MUTANTS, ids=["no_rows", "no_cols", "stoi_clip", "alpha_1", "means_removed"])
def test_bar_catches_mutant(sets, which, kw, bar):
    shift = []
    for fs, r, e in _pairs(sets):
        if which == "estoi":
            shift.append(abs(EX.estoi(r, e, fs, **kw) - EX.estoi(r, e, fs)))
        else:
            shift.append(abs(EX.sisdr(r, e, **kw) - EX.sisdr(r, e)))
    print(which, kw, ["%.3g" % s for s in shift])
    assert max(shift) >= 10 * bar, shift


# ---- 4. argument errors before any device use
def _bpeval(*args):
    r = subprocess.run([BPEVAL] + list(args), capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r                 # (errors: exit(0); success returns 1)
    return r.stdout


def test_bpeval_rejects_a_bad_scores_value(lib, tmp_path):
    (tmp_path / "none.pairs").write_text("")
    for bad in ("bogus", "", "Extended", "basic|extended"):
        assert _bpeval("pairs_list=%s" % (tmp_path / "none.pairs"), "fea_dim=129", "scores=" + bad) == "bpeval: bad value for scores: %s\n" % bad
    # a good value is a key of both modes: the run goes on to its next check
    for good in ("basic", "extended"):
        assert "can not open pairs_list" in _bpeval("pairs_list=%s" % (tmp_path / "nope.pairs"), "fea_dim=129", "scores=" + good)
        assert "need norm_file and initwts_file" in _bpeval("fea_dim=129", "fea_context=3", "layersizes=387,64,129", "scores=" + good)


def _score_ext(lib, n_scores, fs=8000, fea_dim=129):
    lens = np.array([100], np.int32)
    r, e, o = np.zeros(100, np.float32), np.zeros(100, np.float32), np.zeros((1, 8), np.float32)
    fp = C.POINTER(C.c_float)
    return lib.bp_score_waves_ext(0, fea_dim, fs, 1, lens.ctypes.data_as(C.POINTER(C.c_int)), r.ctypes.data_as(fp), e.ctypes.data_as(fp),
                                  n_scores, o.ctypes.data_as(fp))


def test_ext_calls_reject_a_bad_n_scores(lib, pkg):
    for ns in (4, 0, 6, -3, 2):
        assert _score_ext(lib, ns) == -1, ns
        assert b"bp_score_waves_ext: n_scores must be" in lib.bp_last_error()
    # n_scores comes first, then the checks of bp_score_waves in its order
    assert _score_ext(lib, 4, fs=44100) == -1 and b"n_scores" in lib.bp_last_error()
    for ns in (3, 5):
        assert _score_ext(lib, ns, fs=44100) == -1 and b"sample_rate" in lib.bp_last_error()
        assert _score_ext(lib, ns, fea_dim=100) == -1 and b"power of two" in lib.bp_last_error()
    m = np.zeros(1, pkg.MIXTURE_DTYPE)
    s = np.zeros((1, 5), np.float32)
    fp = C.POINTER(C.c_float)
    assert lib.bp_eval_mix_ext(None, 1, m.ctypes.data_as(C.c_void_p), 8000, 0, 0, 4, s.ctypes.data_as(fp), s.ctypes.data_as(fp), None) == -1
    assert b"bp_eval_mix_ext: n_scores" in lib.bp_last_error()
    assert lib.bp_eval_mix_logmmse_ext(None, None, 1, m.ctypes.data_as(C.c_void_p), 8000, 4, s.ctypes.data_as(fp), s.ctypes.data_as(fp), None) == -1
    assert b"bp_eval_mix_logmmse_ext: n_scores" in lib.bp_last_error()
    assert lib.bp_eval_mix_ext(None, 1, m.ctypes.data_as(C.c_void_p), 8000, 0, 0, 5, s.ctypes.data_as(fp), s.ctypes.data_as(fp), None) == -1
    assert b"null handle" in lib.bp_last_error()


def test_constants_and_kernels(lib, pkg):
    assert (pkg.SCORE_ESTOI, pkg.SCORE_SISDR) == (3, 4)
    hdr = open(os.path.join(ROOT, "include", "bp_c_api.h")).read()
    assert "BP_SCORE_ESTOI = 3, BP_SCORE_SISDR = 4, BP_SCORE_EXT_N = 5" in hdr
    data = open(pkg.LIB_PATH, "rb").read()
    for k in ("bp_eval_estoi", "bp_eval_sisdr"):
        assert re.search(rb"_Z\d+" + k.encode() + rb"\w*\.kd", data), k
