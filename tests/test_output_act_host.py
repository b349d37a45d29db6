"""CPU tests of the logistic output layer (bp_set_output, include/bp_c_api.h): the library exports the entry point and checks
its handle, the Python mirror rejects bad values before they reach the library, and the device code holds the logistic
siblings of the three output-layer kernels (fp32 split-K, fp32 plain, bf16) without extra serialised loads."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
BP_ERR_ARG = -1          # include/bp_c_api.h


def test_library_exports_bp_set_output_and_rejects_a_null_handle(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "bp_set_output")
    assert "bp_set_output" in pkg.ABI_SYMBOLS
    for args in ((0, 0, 0), (1, 0, 0), (1, 16, 1)):
        assert lib.bp_set_output(None, *args) == BP_ERR_ARG
        assert b"null handle" in lib.bp_last_error()


class _Stub(object):
    """A BP_GPU whose library must never be reached: every check has to fire in Python."""

    def __init__(self, pkg, sL):
        self.o = pkg.BP_GPU.__new__(pkg.BP_GPU)
        self.o._strict, self.o._h, self.o.layersizes = False, None, [8, 16, sL]

        class NoLib(object):
            def __getattr__(s, name):
                raise AssertionError("the library was called: " + name)
        self.o._lib = NoLib()


@pytest.mark.parametrize("args", [(2, 0, 0), (-1, 0, 0), (1, 0, 2), (1, 0, -1), (0, 3, 0), (0, 0, 1), (1, 33, 0), (1, -1, 0)])
def test_python_mirror_rejects_bad_values_before_the_library(pkg, args):
    s = _Stub(pkg, 33)
    with pytest.raises(pkg.BPError):
        s.o.set_output(*args)


def test_python_mirror_constructor_checks_output_kwargs_before_bp_create(pkg):
    import numpy as np
    ls = [8, 4]
    W = [None, np.zeros((8, 4), np.float32)]
    b = [None, np.zeros(4, np.float32)]
    with pytest.raises(pkg.BPError, match="linear_cols"):      # raised before bp_create: no GPU needed
        pkg.BP_GPU(1, 2, ls, 4, 1.0, 0.5, 0.0, W, b, output_activation=1, output_linear_cols=4)


# mangled-name prefix of each logistic kernel -> the linear sibling it must not be worse than
SIBLINGS = {
    "_Z18bp_out_split_stageI10GemmKernelILi32ELi32ELi64ELi1ELi1ELb1ELb0ELi8EEE":
        "_Z18bp_out_split_stageI10GemmKernelILi32ELi32ELi64ELi1ELi1ELb1ELb0ELi6EEE",      # fp32 split-K + staging
    "_Z7bp_gemmILi32ELi32ELi64ELi1ELi1ELb1ELb0ELi7ELi0EE": "_Z7bp_gemmILi32ELi32ELi64ELi1ELi1ELb1ELb0ELi1ELi0EE",   # fp32 plain 32x32
    "_Z7bp_gemmILi32ELi64ELi64ELi1ELi2ELb1ELb0ELi7ELi0EE": "_Z7bp_gemmILi32ELi64ELi64ELi1ELi2ELb1ELb0ELi1ELi0EE",   # fp32 plain 32x64
    "_Z12bp_gemm_bf16ILi5ELi32ELb1ELb0ELi4EE": "_Z12bp_gemm_bf16ILi1ELi32ELb1ELb0ELi4EE",                           # bf16 split-k
    "_Z12bp_gemm_bf16ILi5ELi32ELb1ELb0ELi1EE": "_Z12bp_gemm_bf16ILi1ELi32ELb1ELb0ELi1EE",                           # bf16 plain
    "_Z12bp_gemm_bf16ILi5ELi64ELb1ELb0ELi1EE": "_Z12bp_gemm_bf16ILi1ELi64ELb1ELb0ELi1EE",
    "_Z12bp_gemm_bf16ILi5ELi128ELb1ELb0ELi1EE": "_Z12bp_gemm_bf16ILi1ELi128ELb1ELb0ELi1EE",
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_logistic_output_kernels_exist_and_drain_no_more_than_their_linear_siblings(tmp_path):
    out = str(tmp_path / "bp_step.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", out,
                           os.path.join(CSRC, "bp_step.hip")], stderr=subprocess.DEVNULL)
    counts, cur, code = {}, None, {}
    for line in open(out):
        m = re.match(r"^(_Z[A-Za-z0-9_]+):", line)
        if m:
            cur = m.group(1); counts[cur] = 0; code[cur] = []
        elif cur:
            code[cur].append(line)
            if "s_waitcnt vmcnt(0)" in line:
                counts[cur] += 1
    shutil.rmtree(str(tmp_path), ignore_errors=True)

    def one(prefix):
        hits = [k for k in counts if k.startswith(prefix)]
        assert len(hits) == 1, (prefix, hits)
        return hits[0]
    for logi, lin in SIBLINGS.items():
        kl, kn = one(logi), one(lin)
        assert counts[kl] <= counts[kn], (kl, counts[kl], kn, counts[kn])
        assert any("v_exp_f32" in s for s in code[kl]), ("no exponential in the logistic kernel", kl)
        assert not any("v_exp_f32" in s for s in code[kn]), ("the linear kernel evaluates an exponential", kn)
