"""CPU tests of the objective scores (no GPU): the float64 restatement in tests/eval_np.py against scipy and against hand-computed
cases, the argument checks of bp_score_waves / bp_eval_mix that come before any device use, the bp_eval_* kernels in the
library's gfx950 code object, and bpeval's checks of keys, values and WAVs."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import eval_np as EN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")
BPEVAL = os.path.join(PKG, "bpeval")
KERNELS = ["bp_eval_resample", "bp_eval_energy", "bp_eval_mask", "bp_eval_compact", "bp_eval_bands", "bp_eval_corr",
           "bp_eval_ssnr", "bp_eval_lsd", "bp_eval_reduce", "bp_eval_trim"]


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH) or not os.path.exists(BPEVAL):
        import __graft_entry__
        __graft_entry__.build()
    return pkg.load_library()


# ---- the restatement
@pytest.mark.parametrize("fs", [8000, 12000, 16000, 48000])
def test_resampler_equals_scipy(fs):
    signal = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(fs).normal(size=2 * fs // 10 + 3)
    p, q = EN.rate_pq(fs)
    y = signal.resample_poly(x, p, q)
    assert y.shape == EN.resample(x, fs).shape
    assert np.abs(EN.resample(x, fs) - y).max() < 1e-12


def test_rates():
    for fs in (8000, 10000, 12000, 16000, 20000, 24000, 32000, 48000):
        assert EN.rate_pq(fs) is not None, fs
    for fs in (44100, 22050, 11025, 96000, 0, -1, 330):
        assert EN.rate_pq(fs) is None, fs


def test_band_table_is_thirdoct():
    assert EN.thirdoct() == EN.BANDS


def test_stoi_identity_scale_and_monotone():
    rng = np.random.default_rng(3)
    r = EN.speech_like(rng, 3 * 16000, 16000)
    assert abs(EN.stoi(r, r, 16000, check_margin=True) - 1.0) < 1e-12
    assert abs(EN.stoi(r, 3 * r, 16000) - 1.0) < 1e-12
    s = [EN.stoi(r, EN.add_noise(rng, r, snr), 16000) for snr in (-5, 0, 5, 10, 20)]
    assert all(a < b for a, b in zip(s, s[1:])), s


def test_ssnr_hand_computed():
    """fs = 400: win = 12, skip = 3; n = 18 gives J = floor(6 - 4) = 2 frames."""
    fs, n = 400, 18
    r = np.arange(1, n + 1, dtype=np.float64)
    e = r.copy()
    e[5] += 2.0                                       # in frame 0 (samples 0..11) and frame 1 (3..14)
    w = 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, 13) / 13))
    want = []
    for j in range(2):
        seg = r[3 * j:3 * j + 12]
        es = ((w * seg) ** 2).sum()
        ed = (w[5 - 3 * j] * 2.0) ** 2
        want.append(min(max(10 * math.log10(es / (ed + EN.EPS) + EN.EPS), -10), 35))
    assert EN.ssnr_frames(r, e, fs).tolist() == pytest.approx(want, rel=1e-15)
    assert EN.ssnr(r, e, fs) == pytest.approx(sum(want) / 2, rel=1e-15)
    assert math.isnan(EN.ssnr(r[:14], e[:14], fs))    # J = floor(14/3 - 4) = 0


def test_ssnr_clamps():
    rng = np.random.default_rng(4)
    r = EN.speech_like(rng, 8000, 8000, gaps=0)
    assert EN.ssnr(r, r, 8000) == 35.0
    z = r.copy()
    z[2000:4000] = 0.0                                # all-zero SSNR frames of r: 10 log10(eps) before the clamp -> -10
    f = EN.ssnr_frames(z, z, 8000)
    win, skip = 240, 60
    zero = [j for j in range(f.size) if not z[j * skip:j * skip + win].any()]
    assert zero and all(f[j] == -10.0 for j in zero)
    assert all(f[j] == 35.0 for j in range(f.size) if j not in zero)


def test_lsd_identity():
    r = EN.speech_like(np.random.default_rng(5), 5000, 8000)
    assert EN.lsd(r, r, 129) == 0.0


# ---- argument checks before any device use
def _score(lib, fea_dim=129, fs=8000, lens=(100,), ref=True, est=True, out=True, sent_len=True):
    lens = np.asarray(lens, np.int32)
    n = int(max(lens.sum(), 1))
    r = np.zeros(n, np.float32)
    e = np.zeros(n, np.float32)
    o = np.zeros((max(len(lens), 1), 3), np.float32)
    fp = C.POINTER(C.c_float)
    return lib.bp_score_waves(0, fea_dim, fs, len(lens), lens.ctypes.data_as(C.POINTER(C.c_int)) if sent_len else None,
                              r.ctypes.data_as(fp) if ref else None, e.ctypes.data_as(fp) if est else None,
                              o.ctypes.data_as(fp) if out else None)


def test_score_waves_rejects_bad_arguments(lib):
    for fs in (44100, 0, -1, 96000, 11025):
        assert _score(lib, fs=fs) == -1, fs
        assert b"sample_rate" in lib.bp_last_error()
    for D in (100, 32, 2049, 0):
        assert _score(lib, fea_dim=D) == -1, D
        assert b"power of two" in lib.bp_last_error()
    assert _score(lib, lens=(100, 0)) == -1
    assert b"empty sentence 1" in lib.bp_last_error()
    assert _score(lib, lens=()) == -1
    for k in ("ref", "est", "out", "sent_len"):
        assert _score(lib, **{k: False}) == -1, k
        assert b"null pointer" in lib.bp_last_error()


def test_eval_mix_rejects_null_handle(lib, pkg):
    m = np.zeros(1, pkg.MIXTURE_DTYPE)
    s = np.zeros((1, 3), np.float32)
    fp = C.POINTER(C.c_float)
    assert lib.bp_eval_mix(None, 1, m.ctypes.data_as(C.c_void_p), 8000, 0, 0, s.ctypes.data_as(fp), s.ctypes.data_as(fp), None) == -1
    assert b"null handle" in lib.bp_last_error()


def test_score_constants(pkg):
    assert (pkg.SCORE_SSNR, pkg.SCORE_LSD, pkg.SCORE_STOI) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "bp_c_api.h")).read()
    assert "BP_SCORE_SSNR = 0, BP_SCORE_LSD = 1, BP_SCORE_STOI = 2, BP_SCORE_N = 3" in hdr


def test_kernels_in_code_object(lib, pkg):
    """the scoring kernels are compiled for gfx950 into the library: the code object carries their descriptors."""
    data = open(pkg.LIB_PATH, "rb").read()
    for k in KERNELS:
        assert re.search(rb"_Z\d+" + k.encode() + rb"\w*\.kd", data), k


# ---- bpeval: bad keys, lists and values are reported (message + exit 0) before any device use
def _write_pcm16(path, x, rate=8000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


@pytest.fixture(scope="module")
def wavs(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("bpeval")
    rng = np.random.default_rng(0)
    for name, n, rate in [("a", 3000, 8000), ("b", 3000, 8000), ("c", 2000, 8000), ("d", 3000, 16000), ("e", 3000, 44100)]:
        _write_pcm16(d / (name + ".wav"), rng.normal(0, 3000, n), rate)
    (d / "bad.wav").write_bytes(b"NOT A WAVE FILE AT ALL")
    (d / "ab.pairs").write_text("%s %s\n" % (d / "a.wav", d / "b.wav"))
    (d / "len.pairs").write_text("%s %s\n" % (d / "a.wav", d / "c.wav"))
    (d / "rate.pairs").write_text("%s %s\n" % (d / "a.wav", d / "d.wav"))
    (d / "mixed.pairs").write_text("%s %s\n%s %s\n" % (d / "a.wav", d / "b.wav", d / "d.wav", d / "d.wav"))
    (d / "cd.pairs").write_text("%s %s\n" % (d / "e.wav", d / "e.wav"))
    (d / "one.pairs").write_text("%s\n" % (d / "a.wav"))
    (d / "good.list").write_text("%s\n%s\n" % (d / "a.wav", d / "c.wav"))
    (d / "mixed.list").write_text("%s\n%s\n" % (d / "a.wav", d / "d.wav"))
    (d / "bad.list").write_text("%s\n" % (d / "bad.wav"))
    (d / "x.norm").write_text("<mean>\n" + "0\n" * 129 + "<inverse std>\n" + "1\n" * 129)
    return d


def _bpeval(*args):
    r = subprocess.run([BPEVAL] + list(args), capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r                 # (errors: exit(0); success returns 1)
    return r.stdout


def test_bpeval_rejects_bad_keys_and_values(wavs):
    good = ["pairs_list=%s" % (wavs / "ab.pairs"), "fea_dim=129"]
    assert "unknown key foo" in _bpeval(*good, "foo=1")
    assert "Format Error" in _bpeval(*good, "fea_dim")
    for bad in ("fea_dim=x", "device=-1", "snr_list=1,a", "snr_list=nan", "mix_per_clean=0", "traincache=-3", "compute=fp16",
                "wave_target=irm", "output_act=tanh", "init_randem_seed=-1", "out_col=-2", "layersizes=3,x"):
        k = bad.split("=")[0]
        assert "bad value for " + k in _bpeval(*good, bad), bad
    assert "power of two" in _bpeval(good[0], "fea_dim=100")
    assert "pairs_list takes only" in _bpeval(*good, "fea_context=3")


def test_bpeval_rejects_bad_pairs(wavs):
    def pairs(name):
        return _bpeval("pairs_list=%s" % (wavs / name), "fea_dim=129")
    assert "differ in length" in pairs("len.pairs")
    assert "differ in sample rate" in pairs("rate.pairs")
    assert "the others 8000 Hz" in pairs("mixed.pairs")
    assert "not a scoring rate" in pairs("cd.pairs")
    assert "needs a reference and an estimate" in pairs("one.pairs")
    assert "can not open pairs_list" in pairs("nope.pairs")


def test_bpeval_rejects_bad_test_sets(wavs):
    net = ["fea_dim=129", "fea_context=3", "targ_offset=1", "layersizes=387,64,129", "norm_file=%s" % (wavs / "x.norm"),
           "initwts_file=%s" % (wavs / "nope.wts"), "traincache=1000"]
    good = "clean_list=%s" % (wavs / "good.list")
    assert "the others 8000 Hz" in _bpeval("clean_list=%s" % (wavs / "mixed.list"), "noise_list=%s" % (wavs / "good.list"), *net)
    assert "the others 8000 Hz" in _bpeval(good, "noise_list=%s" % (wavs / "mixed.list"), *net)
    assert "not a RIFF/WAVE file" in _bpeval(good, "noise_list=%s" % (wavs / "bad.list"), *net)
    assert "noise_list is not given" in _bpeval(good, *net)
    assert "out_col + fea_dim exceeds" in _bpeval(good, "noise_list=%s" % (wavs / "good.list"), *net, "out_col=1")
    assert "layersizes[0] must be" in _bpeval(good, "noise_list=%s" % (wavs / "good.list"), *net[:3], "layersizes=300,64,129", *net[4:])
    assert "can not open initial weights file" in _bpeval(good, "noise_list=%s" % (wavs / "good.list"), *net)
