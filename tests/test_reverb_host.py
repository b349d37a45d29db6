"""CPU tests of the reverberant corpus entries (no GPU): the restatement in tests/reverb_np.py against np.convolve, the host-only
entry points bp_mix_rir_delay / bp_mix_reverb_pairs against it, the argument checks that come before any device use, the kernel
in the library's gfx950 code object and bpmix's checks of rir_list."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reverb_np as RV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")
BPMIX = os.path.join(PKG, "bpmix")
KERNELS = ["bp_mix_reverb_fir"]
SYMBOLS = ["bp_set_mix_reverb", "bp_reverb_waves", "bp_mix_rir_delay", "bp_mix_reverb_pairs"]


@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH) or not os.path.exists(BPMIX):
        import __graft_entry__
        __graft_entry__.build()
    return pkg.load_library()


def _conv(s, h, d, upto):
    """np.convolve in float64 of s with the taps 0 .. upto, read at the direct path."""
    full = np.convolve(np.asarray(s, np.float64), np.asarray(h, np.float64)[:upto + 1])
    full = np.concatenate([full, np.zeros(d + len(s))])
    return full[d:d + len(s)]


# ---- the restatement
@pytest.mark.parametrize("n,Lh,pos,early", [(300, 1, 0, 0), (300, 64, 0, 5), (1000, 257, 100, 40), (50, 400, 399, 0), (700, 33, 16, 1000)])
def test_restatement_matches_convolve(n, Lh, pos, early):
    rng = np.random.default_rng(n + Lh)
    s = np.round(rng.normal(0, 3000, n)).astype(np.float32)
    h = rng.normal(0, 3000, Lh).astype(np.float32)
    h[pos] = 4 * np.abs(h).max()
    assert RV.delay(h) == pos
    r, e = RV.reverb(s, h, early)
    for got, upto in ((r, Lh - 1), (e, min(Lh - 1, pos + early))):
        want = _conv(s, h, pos, upto).astype(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))), "more than 1 fp32 ulp from np.convolve"


@pytest.mark.parametrize("n,Lh", [(500, 7), (64, 300), (2049, 257)])
def test_restatement_exact_on_exact_data(n, Lh):
    rng = np.random.default_rng(n)
    s, h = RV.exact_case(rng, n, Lh)
    d = RV.delay(h)
    r, e = RV.reverb(s, h, 3)
    assert np.array_equal(r.astype(np.float64), _conv(s, h, d, Lh - 1))
    assert np.array_equal(e.astype(np.float64), _conv(s, h, d, min(Lh - 1, d + 3)))


def test_restatement_simple_responses():
    rng = np.random.default_rng(0)
    s = np.round(rng.normal(0, 3000, 100)).astype(np.float32)
    for h, want, d in (([1.0], s, 0), ([0.0, 0.0, 1.0], s, 2), ([0.5], s / 2, 0)):
        r, e = RV.reverb(s, np.array(h, np.float32), 0)
        assert RV.delay(h) == d
        assert np.array_equal(r.view(np.uint32), want.view(np.uint32)) and np.array_equal(e.view(np.uint32), want.view(np.uint32))
    h = rng.normal(0, 1, 20).astype(np.float32)
    for early in (20, 21, 1000):
        r, e = RV.reverb(s, h, early)
        assert np.array_equal(r.view(np.uint32), e.view(np.uint32))
    r, es = RV.reverb(s, h, [0, 3, 50])
    for t, e in zip([0, 3, 50], es):
        assert np.array_equal(e.view(np.uint32), RV.reverb(s, h, t)[1].view(np.uint32))
    assert RV.delay([1.0, -3.0, 3.0, 2.0, -3.0]) == 1, "the first of tied maxima"
    assert RV.delay([0.0, 0.0]) == 0


# ---- host-only entry points
def test_delay_and_pairs_match_restatement(lib, pkg):
    rng = np.random.default_rng(1)
    for n in (1, 2, 17, 4000, RV.MAX_TAPS):
        h = rng.normal(0, 1, n).astype(np.float32)
        assert pkg.rir_delay(h) == RV.delay(h)
    assert pkg.rir_delay([1.0, -3.0, 3.0, 2.0, -3.0]) == 1
    assert pkg.rir_delay([0.0, 0.0, 0.0]) == 0
    for seed, n_clean, n_rir in ((0, 1, 1), (345, 50, 3), (2 ** 40 + 9, 200, 7), (20261016, 9, 1000)):
        got = pkg.mix_reverb_pairs(seed, n_clean, n_rir)
        assert got.dtype == np.int32 and np.array_equal(got, RV.pairs(seed, n_clean, n_rir))
        assert np.all((got >= 0) & (got < n_rir))
    assert not np.array_equal(pkg.mix_reverb_pairs(1, 100, 5), pkg.mix_reverb_pairs(2, 100, 5))
    for args in ((1, 0, 3), (1, 3, 0)):
        with pytest.raises(pkg.BPError, match="status -1"):
            pkg.mix_reverb_pairs(*args)
    assert lib.bp_mix_reverb_pairs(1, 3, 3, None) == -1
    d = C.c_int()
    h = np.ones(4, np.float32)
    fp = h.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.bp_mix_rir_delay(None, 4, C.byref(d)) == -1 and lib.bp_mix_rir_delay(fp, 4, None) == -1
    assert lib.bp_mix_rir_delay(fp, 0, C.byref(d)) == -1
    big = np.ones(RV.MAX_TAPS + 1, np.float32)
    assert lib.bp_mix_rir_delay(big.ctypes.data_as(C.POINTER(C.c_float)), big.size, C.byref(d)) == -1
    h[2] = np.inf
    assert lib.bp_mix_rir_delay(fp, 4, C.byref(d)) == -1


def _waves_rc(lib, sent_len, pcm, sent_rir, rir_len, rir_pcm, early_taps=0, n_sent=None, n_rir=None, null=()):
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    sl, sr, rl = (np.array(x, np.int32) for x in (sent_len, sent_rir, rir_len))
    pcm, rir_pcm = np.array(pcm, np.float32), np.array(rir_pcm, np.float32)
    out_r, out_e = np.zeros(max(pcm.size, 1), np.float32), np.zeros(max(pcm.size, 1), np.float32)
    a = dict(sent_len=sl.ctypes.data_as(ip), pcm=pcm.ctypes.data_as(fp), sent_rir=sr.ctypes.data_as(ip), rir_len=rl.ctypes.data_as(ip),
             rir_pcm=rir_pcm.ctypes.data_as(fp), out_rev=out_r.ctypes.data_as(fp), out_early=out_e.ctypes.data_as(fp))
    for k in null:
        a[k] = None
    return lib.bp_reverb_waves(0, len(sl) if n_sent is None else n_sent, a["sent_len"], a["pcm"], a["sent_rir"],
                               len(rl) if n_rir is None else n_rir, a["rir_len"], a["rir_pcm"], early_taps, a["out_rev"], a["out_early"])


def test_argument_errors_before_any_device(lib, pkg):
    """every one of these is BP_ERR_ARG (-1) on a machine without a GPU: the checks come before the device is looked for"""
    r = pkg.BPMixReverb()
    assert lib.bp_set_mix_reverb(None, C.byref(r)) == -1
    assert b"null handle" in lib.bp_last_error()
    assert lib.bp_set_mix_reverb(None, None) == -1
    good = dict(sent_len=[3, 2], pcm=[1, 2, 3, 4, 5], sent_rir=[0, 1], rir_len=[2, 1], rir_pcm=[1, 0.5, 2])
    for k in ("sent_len", "pcm", "sent_rir", "rir_len", "rir_pcm"):
        assert _waves_rc(lib, null=(k,), **good) == -1, k
    assert _waves_rc(lib, null=("out_rev", "out_early"), **good) == -1
    assert _waves_rc(lib, n_sent=0, **good) == -1
    assert _waves_rc(lib, n_rir=0, **good) == -1
    assert _waves_rc(lib, early_taps=-1, **good) == -1
    for bad in (dict(sent_len=[3, 0]), dict(sent_len=[3, -2]), dict(rir_len=[0, 1]), dict(rir_len=[2, -1]), dict(sent_rir=[0, 2]),
                dict(sent_rir=[-1, 1]), dict(rir_pcm=[1, np.nan, 2]), dict(rir_pcm=[1, 0.5, np.inf])):
        assert _waves_rc(lib, **dict(good, **bad)) == -1, bad
    long_h = np.ones(RV.MAX_TAPS + 1, np.float32)
    assert _waves_rc(lib, [3], [1, 2, 3], [0], [long_h.size], long_h) == -1
    assert b"65536" in lib.bp_last_error()


def test_kernel_in_code_object_and_symbols_exported(lib, pkg):
    data = open(pkg.LIB_PATH, "rb").read()
    for k in KERNELS:                                   # kernel descriptor of the (mangled) kernel name
        assert re.search(rb"_Z\d+" + k.encode() + rb"\w*\.kd", data), k
    for s in SYMBOLS:
        assert s in pkg.ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.bp_abi_version() == 5


# ---- bpmix: rir_list is checked (message + exit 0, the reference convention) before any device use
def _write_pcm16(path, x, rate=8000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(x, np.int16).tobytes())


@pytest.fixture(scope="module")
def lists(lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("bpmix_rir")
    rng = np.random.default_rng(0)
    for i, n in enumerate([3000, 800]):
        _write_pcm16(d / ("c%d.wav" % i), rng.normal(0, 3000, n))
    _write_pcm16(d / "h8.wav", [0, 20000, 3000, -1000])
    _write_pcm16(d / "h16.wav", [0, 20000, 3000, -1000], rate=16000)
    (d / "good.list").write_text("%s\n%s\n" % (d / "c0.wav", d / "c1.wav"))
    (d / "rir.list").write_text("%s\n" % (d / "h8.wav"))
    (d / "rir16.list").write_text("%s\n%s\n" % (d / "h8.wav", d / "h16.wav"))
    (d / "missing.list").write_text("%s\n" % (d / "nothere.wav"))
    (d / "empty.list").write_text("\n")
    return d


def _bpmix(*args):
    r = subprocess.run([BPMIX] + list(args), capture_output=True, text=True, timeout=60, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r                 # (errors: exit(0); success returns 1)
    return r.stdout


def test_bpmix_rejects_bad_rir_lists(lists):
    base = ["clean_list=%s" % (lists / "good.list"), "noise_list=%s" % (lists / "good.list"), "fea_dim=129", "norm_out=%s" % (lists / "x.norm")]
    assert "can not open rir_list" in _bpmix(*base, "rir_list=%s" % (lists / "nope.list"))
    assert "nothere.wav" in _bpmix(*base, "rir_list=%s" % (lists / "missing.list"))
    assert "lists no wav file" in _bpmix(*base, "rir_list=%s" % (lists / "empty.list"))
    assert "16000 Hz, the clean sentences 8000 Hz" in _bpmix(*base, "rir_list=%s" % (lists / "rir16.list"))
    assert "is not reverberant or early" in _bpmix(*base, "rir_list=%s" % (lists / "rir.list"), "reverb_target=dry")
    for bad in ("early_ms=-1", "early_ms=x", "early_ms=nan"):
        assert "bad value for early_ms" in _bpmix(*base, "rir_list=%s" % (lists / "rir.list"), bad), bad
    assert not os.path.exists(lists / "x.norm")
