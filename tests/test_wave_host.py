"""CPU tests of the signal layer: argument checks of bp_wave_lps / bp_enhance_waves that come before any device use, the
command-line checks of bpfeat / bpenhance (message + exit 0, reference convention) for missing keys and malformed WAV files,
and the new kernels in the library's gfx950 code object."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dnn-for-speech-enhancement_amd")
BPFEAT = os.path.join(PKG, "bpfeat")
BPENHANCE = os.path.join(PKG, "bpenhance")
KERNELS = ["bp_wave_analysis", "bp_wave_nat", "bp_wave_synthesis", "bp_wave_overlap"]


@pytest.fixture(scope="module")
def lib(pkg):
    if not (os.path.exists(pkg.LIB_PATH) and os.path.exists(BPFEAT) and os.path.exists(BPENHANCE)):
        import __graft_entry__
        __graft_entry__.build()
    return pkg.load_library()


def _lps(lib, fea_dim, lens, pcm=True, out=True):
    lens = np.asarray(lens, np.int32)
    x = np.zeros(max(int(lens.sum()), 1), np.float32)
    y = np.zeros(1 << 16, np.float32)
    fp = C.POINTER(C.c_float)
    return lib.bp_wave_lps(0, fea_dim, len(lens), lens.ctypes.data_as(C.POINTER(C.c_int)),
                           x.ctypes.data_as(fp) if pcm else None, y.ctypes.data_as(fp) if out else None)


@pytest.mark.parametrize("fea_dim", [0, 32, 100, 130, 1026, 2049])
def test_wave_lps_rejects_fft_sizes(lib, fea_dim):
    assert _lps(lib, fea_dim, [500]) == -1
    assert b"power of two" in lib.bp_last_error()


def test_wave_lps_rejects_empty_sentence_and_nulls(lib):
    assert _lps(lib, 129, [300, 0, 20]) == -1
    assert b"empty sentence 1" in lib.bp_last_error()
    assert _lps(lib, 129, [300], pcm=False) == -1
    assert _lps(lib, 129, [300], out=False) == -1
    assert lib.bp_wave_lps(0, 129, 1, None, None, None) == -1
    assert lib.bp_wave_lps(0, 129, 0, None, None, None) == -1


def test_enhance_waves_rejects_null_handle_or_chunk(lib, pkg):
    c = pkg.BPWaveChunk()
    out = np.zeros(16, np.float32)
    fp = C.POINTER(C.c_float)
    assert lib.bp_enhance_waves(None, 129, C.byref(c), out.ctypes.data_as(fp), None) == -1
    assert b"null handle or chunk" in lib.bp_last_error()
    assert lib.bp_enhance_waves(None, 129, None, out.ctypes.data_as(fp), None) == -1


def test_wave_kernels_in_gfx950_code_object(lib, tmp_path):
    fb = str(tmp_path / "fatbin")
    subprocess.check_call(["/opt/rocm/llvm/bin/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin",
                           os.path.join(PKG, "libbp_hip.so"), fb])
    data = open(fb, "rb").read()
    assert b"gfx950" in data
    for k in KERNELS:                                   # kernel descriptor of the (mangled) kernel name
        assert re.search(rb"_Z\d+" + k.encode() + rb"\w*\.kd", data), k


# ---- command-line tools
def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r
    return r.stdout


def _riff(fmt_body, data, declared=None):
    fmt = b"fmt " + struct.pack("<I", len(fmt_body)) + fmt_body
    dat = b"data" + struct.pack("<I", len(data) if declared is None else declared) + data
    body = b"WAVE" + fmt + dat
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _fmt(tag, ch, rate, bits):
    return struct.pack("<HHIIHH", tag, ch, rate, rate * ch * bits // 8, ch * bits // 8, bits)


MALFORMED = {
    "stereo": _riff(_fmt(1, 2, 8000, 16), b"\0" * 400),
    "pcm24": _riff(_fmt(1, 1, 8000, 24), b"\0" * 300),
    "truncated": _riff(_fmt(1, 1, 8000, 16), b"\0" * 100, declared=4000),
    "not_riff": b"JUNK" + b"\0" * 60,
}
MESSAGES = {"stereo": "channels", "pcm24": "bits", "truncated": "truncated", "not_riff": "not a RIFF"}


def test_tools_report_missing_keys(lib):
    assert "need wav_list" in _run(BPFEAT, "fea_dim=129")
    assert "power of two" in _run(BPFEAT, "wav_list=x", "out_file=y", "fea_dim=100")
    assert "need layersizes" in _run(BPENHANCE, "fea_dim=129")
    assert "need norm_file" in _run(BPENHANCE, "layersizes=129,64,129", "fea_dim=129")
    assert "need wav_list, or in_wav" in _run(BPENHANCE, "layersizes=129,64,129", "fea_dim=129", "norm_file=n", "initwts_file=w")


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_tools_reject_malformed_wav(lib, tmp_path, case):
    bad = tmp_path / (case + ".wav")
    bad.write_bytes(MALFORMED[case])
    lst = tmp_path / "list"
    lst.write_text("%s\n" % bad)
    out = _run(BPFEAT, "wav_list=%s" % lst, "out_file=%s" % (tmp_path / "o.pfile"), "fea_dim=129")
    assert str(bad) in out and MESSAGES[case] in out, out
    assert not (tmp_path / "o.pfile").exists()
    out = _run(BPENHANCE, "layersizes=129,64,129", "fea_dim=129", "norm_file=n", "initwts_file=w", "in_wav=%s" % bad,
               "out_wav=%s" % (tmp_path / "e.wav"))
    assert str(bad) in out and MESSAGES[case] in out, out
    assert not (tmp_path / "e.wav").exists()
