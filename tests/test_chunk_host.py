"""The resident chunk's record (csrc/bp_chunk.h: the one transition that makes a chunk resident, the copy-stream handshake of an
upload, the preconditions of the calls that read the chunk, unpad_rows and sq_err_sum) on its own: tests/cpp/chunk_driver.cc is a
stand-alone program that stands logging functions in for the runtime calls the header names, built with
-fsanitize=address,undefined in the manner of test_mem_host.py and run on the CPU.  It exits non-zero on the first call order,
state, status, message or sum that is not what the header's invariants say; ASan's leak check at exit is part of the assertion."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "csrc")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
BAD_WORDS = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "Segmentation fault", "core dumped")


def test_resident_chunk_record_under_asan(tmp_path):
    exe = str(tmp_path / "chunk_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "chunk_driver.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    txt = r.stdout + r.stderr
    for w in BAD_WORDS:
        assert w not in txt, txt[-3000:]
    assert r.returncode == 0, (r.returncode, txt[-2000:])
    assert "handshake order, transition, preconditions and the way out agree" in txt, txt


def test_each_block_of_the_resident_chunk_is_written_once():
    """One site each under csrc: the invalidation of a pre-staged tile, the missing-targets message, the ignored-remainder line of the
    library and the CV accumulation (host/bptrain.cpp keeps its own printf: it is a tool, not the library)."""
    texts = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}
    for needle in ("gen++", "uploaded without targets", "is ignored.", "squared_err + e * e", "outside the resident chunk"):
        sites = [(f, t.count(needle)) for f, t in texts.items() if needle in t]
        assert sum(n for _, n in sites) == 1, (needle, sites)
