"""The holders of csrc/bp_mem.h (Buf, Event, Stream, grow_all, Layout -- who frees the library's device memory, pinned memory and
events) on their own: tests/cpp/mem_driver.cc is a stand-alone program that stands counting functions in for the runtime calls the
header uses, built with -fsanitize=address,undefined in the manner of test_stream_core_host.py and run on the CPU.  It exits
non-zero on the first capacity, call order, balance or offset that is not what the policy says; ASan's leak check at exit is part
of the assertion (every stand-in allocation is a heap block)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "csrc")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
BAD_WORDS = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "Segmentation fault", "core dumped")


def test_mem_holders_under_asan(tmp_path):
    exe = str(tmp_path / "mem_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "mem_driver.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    txt = r.stdout + r.stderr
    for w in BAD_WORDS:
        assert w not in txt, txt[-3000:]
    assert r.returncode == 0, (r.returncode, txt[-2000:])
    assert "holders balance, grow policy and layout agree" in txt, txt
