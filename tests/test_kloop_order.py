"""The order of the fp32 GEMM's k-loop as a host unit (no GPU): tests/cpp/kloop_order_driver.cc enumerates, from the constexpr index
functions GemmCfg::step itself addresses LDS and its accumulator chains with (csrc/bp_kernels.h: step_row, step_chain, NK), the
(wave group, chain, k) triples a workgroup multiplies for 1 .. 9 k-tiles in every tile configuration the step dispatches, and
compares them element for element with the plain loop over BK-deep tiles written out without them.  That is the bit-identity
argument of any rescheduling of the loop, as code.  The same driver runs once more under AddressSanitizer and UBSan (host code
only, a program of its own)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "kloop_order_driver.cc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def _build(exe, extra):
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC] + extra
                          + ["-o", exe, DRIVER])


def test_the_k_loop_multiplies_in_the_order_of_the_plain_loop(tmp_path):
    exe = str(tmp_path / "kloop_order_driver")
    _build(exe, [])
    out = subprocess.check_output([exe], universal_newlines=True)
    assert "in the order of the plain loop" in out, out


def test_the_driver_is_clean_under_the_host_sanitizers(tmp_path):
    """The stand-alone driver, host side compiled with -fsanitize=address,undefined; it is its own program, nothing is preloaded."""
    exe = str(tmp_path / "kloop_order_driver_san")
    _build(exe, ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, env=env)
    assert p.returncode == 0 and "in the order of the plain loop" in p.stdout, p.stdout
