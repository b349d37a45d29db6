"""CPU tests of the training mixtures (no GPU): bp_mix_plan / bp_mix_shuffle against the restatement in tests/mix_np.py, the
argument checks that come before any device use, and the new kernels in the library's gfx950 code object."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mix_np as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")
KERNELS = ["bp_mix_gain", "bp_mix_pcm", "bp_mix_targets", "bp_mix_tables"]


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return pkg.load_library()


@pytest.mark.parametrize("seed,n_clean,per_clean,noise_lens,snrs", [
    (0, 5, 1, [1000], [0.0]),
    (1, 7, 3, [5, 17, 100000, 3], [-5, 0, 5, 10, 15, 20]),
    (345, 13, 2, [40000, 2 ** 31 + 11], [-10.0, 30.0]),
    (2 ** 40 + 9, 1, 9, [1, 2, 3, 4, 5, 6, 7], [2.5, -2.5, 7.0]),
])
def test_plan_matches_restatement(lib, pkg, seed, n_clean, per_clean, noise_lens, snrs):
    got = pkg.mix_plan(seed, n_clean, per_clean, noise_lens, snrs)
    ref = MX.plan(seed, n_clean, per_clean, noise_lens, snrs)
    assert got.dtype == pkg.MIXTURE_DTYPE and got.size == len(ref)
    assert [tuple(x) for x in got.tolist()] == [(c, n, o, float(s)) for c, n, o, s in ref]
    assert np.all((got["offset"] >= 0) & (got["offset"] < np.asarray(noise_lens)[got["noise"]]))
    assert np.all(np.isin(got["snr_db"], np.asarray(snrs, np.float32)))
    assert sorted(got["clean"].tolist()) == [c for c in range(n_clean) for _ in range(per_clean)]
    again = pkg.mix_plan(seed, n_clean, per_clean, noise_lens, snrs)
    assert got.tobytes() == again.tobytes()
    if n_clean * per_clean > 3:
        assert got.tobytes() != pkg.mix_plan(seed + 1, n_clean, per_clean, noise_lens, snrs).tobytes()


@pytest.mark.parametrize("seed,stream,n", [(0, 0, 1), (1, 0, 2), (7, 3, 1000), (345, 11, 37), (2 ** 63 + 5, 2 ** 32 - 1, 500)])
def test_shuffle_matches_restatement(lib, pkg, seed, stream, n):
    got = pkg.mix_shuffle(seed, stream, n)
    assert np.array_equal(got, MX.shuffle(seed, stream, n))
    assert np.array_equal(np.sort(got), np.arange(n))
    if n > 10:
        assert not np.array_equal(got, pkg.mix_shuffle(seed, stream + 1, n))
        assert not np.array_equal(got, pkg.mix_shuffle(seed + 1, stream, n))


def test_plan_and_shuffle_reject_bad_arguments(lib, pkg):
    for args in [(1, 0, 1, [10], [0.0]), (1, 2, 0, [10], [0.0]), (1, 2, 1, [], [0.0]), (1, 2, 1, [10], []),
                 (1, 2, 1, [0], [0.0]), (1, 2, 1, [2 ** 32], [0.0]), (1, 2, 1, [10], [float("nan")]), (1, 2, 1, [10], [float("inf")])]:
        with pytest.raises(pkg.BPError, match="status -1"):
            pkg.mix_plan(*args)
    assert lib.bp_mix_shuffle(1, 0, -1, None) == -1
    assert lib.bp_mix_shuffle(1, 0, 5, None) == -1


def test_calls_reject_null_handle(lib, pkg):
    c = pkg.BPMixCorpus()
    assert lib.bp_set_mix_corpus(None, C.byref(c)) == -1
    assert b"null handle" in lib.bp_last_error()
    m = np.zeros(1, pkg.MIXTURE_DTYPE)
    e = C.c_float()
    assert lib.bp_train_mix(None, 1, m.ctypes.data_as(C.c_void_p), None) == -1
    assert lib.bp_cv_mix(None, 1, m.ctypes.data_as(C.c_void_p), C.byref(e)) == -1
    assert lib.bp_mix_features(None, 1, m.ctypes.data_as(C.c_void_p), None, None, None, None, None) == -1


def test_mixture_struct_layout(pkg):
    class Mixture(C.Structure):
        _fields_ = [("clean", C.c_int), ("noise", C.c_int), ("offset", C.c_int64), ("snr_db", C.c_float)]
    assert C.sizeof(Mixture) == pkg.MIXTURE_DTYPE.itemsize
    for name, _ in Mixture._fields_:
        assert getattr(Mixture, name).offset == pkg.MIXTURE_DTYPE.fields[name][1]


def test_kernels_in_code_object(lib, pkg):
    """the new kernels are compiled for gfx950 into the library: the code object carries their descriptors."""
    data = open(pkg.LIB_PATH, "rb").read()
    for k in KERNELS:                                   # kernel descriptor of the (mangled) kernel name
        assert re.search(rb"_Z\d+" + k.encode() + rb"\w*\.kd", data), k


# ---- bpmix: bad keys, lists and values are reported (message + exit 0, the reference convention) before any device use
BPMIX = os.path.join(PKG, "bpmix")


def _write_pcm16(path, x, rate=8000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


@pytest.fixture(scope="module")
def bpmix(lib, tmp_path_factory):
    if not os.path.exists(BPMIX):
        import __graft_entry__
        __graft_entry__.build()
    d = tmp_path_factory.mktemp("bpmix")
    rng = np.random.default_rng(0)
    for i, n in enumerate([3000, 800]):
        _write_pcm16(d / ("c%d.wav" % i), rng.normal(0, 3000, n))
    (d / "bad.wav").write_bytes(b"NOT A WAVE FILE AT ALL")
    (d / "good.list").write_text("%s\n%s\n" % (d / "c0.wav", d / "c1.wav"))
    (d / "bad.list").write_text("%s\n" % (d / "bad.wav"))
    (d / "missing.list").write_text("%s\n" % (d / "nothere.wav"))
    (d / "empty.list").write_text("\n")
    return d


def _bpmix(*args):
    import subprocess
    r = subprocess.run([BPMIX] + list(args), capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r                 # (errors: exit(0); success returns 1)
    return r.stdout


def test_bpmix_rejects_bad_keys_and_values(bpmix):
    good = ["clean_list=%s" % (bpmix / "good.list"), "noise_list=%s" % (bpmix / "good.list"), "fea_dim=129"]
    assert "unknown key foo" in _bpmix(*good, "foo=1")
    assert "Format Error" in _bpmix(*good, "fea_dim")
    for bad in ("snr_list=", "snr_list=1,a", "snr_list=nan", "snr_list=0,inf", "lrate=x", "mix_per_clean=0", "traincache=-3",
                "compute=fp16", "output_act=tanh", "init_randem_seed=-1", "gpu_used=2"):
        k = bad.split("=")[0]
        assert "bad value for " + k in _bpmix(*good, bad), bad
    assert "is not lps, irm, ibm, lps+irm or lps+ibm" in _bpmix(*good, "target=mask")
    assert "power of two" in _bpmix(*good[:2], "fea_dim=100")


def test_bpmix_rejects_bad_lists(bpmix):
    tail = ["fea_dim=129", "norm_out=%s" % (bpmix / "x.norm")]
    assert "can not open clean_list" in _bpmix("clean_list=%s" % (bpmix / "nope.list"), "noise_list=%s" % (bpmix / "good.list"), *tail)
    assert "not a RIFF/WAVE file" in _bpmix("clean_list=%s" % (bpmix / "bad.list"), "noise_list=%s" % (bpmix / "good.list"), *tail)
    assert "nothere.wav" in _bpmix("clean_list=%s" % (bpmix / "good.list"), "noise_list=%s" % (bpmix / "missing.list"), *tail)
    assert "lists no wav file" in _bpmix("clean_list=%s" % (bpmix / "good.list"), "noise_list=%s" % (bpmix / "empty.list"), *tail)
    assert "noise_list is not given" in _bpmix("clean_list=%s" % (bpmix / "good.list"), *tail)
    train = ["clean_list=%s" % (bpmix / "good.list"), "noise_list=%s" % (bpmix / "good.list"), "fea_dim=129", "fea_context=3",
             "numlayers=3", "layersizes=387,64,129", "traincache=1000", "bunchsize=32", "norm_file=%s" % (bpmix / "x.norm"),
             "outwts_file=%s" % (bpmix / "o.wts"), "log_file=%s" % (bpmix / "o.log")]
    assert "cv_clean_list is not given" in _bpmix(*train)
    assert "layersizes[last] must be 258" in _bpmix(*train, "target=lps+ibm")
    assert "layersizes[0] must be" in _bpmix(*train[:4], "numlayers=3", "layersizes=300,64,129", *train[6:])
    assert "can not open normalization file" in _bpmix(*train, "cv_clean_list=%s" % (bpmix / "good.list"))
    assert not os.path.exists(bpmix / "x.norm") and not os.path.exists(bpmix / "o.wts")
