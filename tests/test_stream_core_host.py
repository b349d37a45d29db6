"""The stream core (csrc/bp_stream_core.h: counts, carry, push checks -- what bp_stream.hip and bp_classic.hip share) on its own:
tests/cpp/stream_core_driver.cc is a stand-alone program of the header's host part, built with -fsanitize=address,undefined in the
manner of test_sanitizers.py and run on the CPU.  It plays sentences through both parameterisations and every push schedule and
exits non-zero on the first frame, carry or count that is not what the padded sentence says."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "csrc")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
BAD_WORDS = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "Segmentation fault", "core dumped")


def test_stream_core_under_asan(tmp_path):
    exe = str(tmp_path / "stream_core_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "stream_core_driver.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    txt = r.stdout + r.stderr
    for w in BAD_WORDS:
        assert w not in txt, txt[-3000:]
    assert r.returncode == 0, (r.returncode, txt[-2000:])
    assert "counts and" in txt and "pushes agree" in txt, txt
