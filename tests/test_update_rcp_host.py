"""The reciprocal the momentum update may multiply by, as a host unit (no GPU).  exact_rdiv (csrc/bp_handle.h) gives the kernels
rdiv = 1/ndiv where `g * rdiv` is `g / ndiv` to the bit and 0 -- keep the IEEE division -- everywhere else;
tests/cpp/update_rcp_driver.cc prints it for a table of divisors (every 2^k, k = 0 .. 24; 3, 96, 100, 384, 768, 2^24 + 2; 0 and
negative values) and checks the edges itself.  Here the table is read back: a power of two must give exactly the float 1/ndiv,
everything else 0; and numpy shows, on more than a million random float32 bit patterns with subnormals, infinities and both zeros
among them, that for every power of two of the table the product and the quotient are the same words, and that for the other
divisors they are not (which is why those keep the division).  The same driver runs once more under AddressSanitizer and UBSan
(host code only, a program of its own)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "dnn-for-speech-enhancement_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "update_rcp_driver.cc")
DONE = "other divisors keep the division"

POW2 = [float(2 ** k) for k in range(25)]
OTHER = [3.0, 96.0, 100.0, 384.0, 768.0, float(2 ** 24 + 2), 0.0, -256.0, -3.0]

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def _build(exe, extra):
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC] + extra
                          + ["-o", exe, DRIVER])


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{ndiv (float32): rdiv (float32)} as the driver printed it."""
    exe = str(tmp_path_factory.mktemp("rcp") / "update_rcp_driver")
    _build(exe, [])
    out = subprocess.check_output([exe], universal_newlines=True)
    assert DONE in out, out
    t = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) == 4 and f[0] == "ndiv" and f[2] == "rdiv":
            n, r = (np.array([int(x, 16)], np.uint32).view(np.float32)[0] for x in (f[1], f[3]))
            t[float(n)] = r
    return t


def _words(n, seed):
    """n random float32 bit patterns (every exponent, so one in 256 is subnormal or zero and one in 256 infinite or NaN), and in
    front of them the words a shift of the exponent is most likely to get wrong."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    sub = rng.integers(0, 1 << 23, size=n // 16, dtype=np.uint64).astype(np.uint32) | (rng.integers(0, 2, size=n // 16, dtype=np.uint64).astype(np.uint32) << 31)
    low = (rng.integers(0, 1 << 23, size=n // 16, dtype=np.uint64) | (rng.integers(1, 26, size=n // 16, dtype=np.uint64) << 23)).astype(np.uint32)  # quotients that land among the subnormals
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x00800001, 0x7F7FFFFF, 0xFF7FFFFF,
                     0x7F800000, 0xFF800000, 0x3F800000], np.uint32)
    return np.concatenate([edge, sub, low, w]).view(np.float32)


def _unequal(a, b):
    """words that differ, NaN payloads aside"""
    return int(np.count_nonzero((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))))


def test_the_table_is_the_reciprocal_for_powers_of_two_and_zero_otherwise(table):
    assert sorted(table) == sorted(set(POW2 + OTHER)), sorted(table)
    for n in POW2:
        r = table[n]
        assert r.dtype == np.float32 and r == np.float32(1.0) / np.float32(n) and float(r) * n == 1.0, (n, r)
    for n in OTHER:
        assert table[n].view(np.uint32) == 0, (n, table[n])


def test_the_product_is_the_quotient_to_the_bit_for_every_power_of_two(table):
    g = _words(1 << 20, seed=18)
    assert g.size >= 1 << 20 and np.isinf(g).any() and (g == 0).any() and np.signbit(g[g == 0]).any()
    assert np.count_nonzero((np.abs(g) < np.float32(2.0 ** -126)) & (g != 0)) > 1 << 16          # subnormal operands
    with np.errstate(all="ignore"):
        for n in POW2:
            q, p = g / np.float32(n), g * table[n]
            assert q.dtype == np.float32 and p.dtype == np.float32
            assert _unequal(p, q) == 0, (n, _unequal(p, q))
            if n > 1:
                assert np.count_nonzero((np.abs(q) < np.float32(2.0 ** -126)) & (q != 0)) > 1 << 16, n      # ... and subnormal quotients


def test_the_other_divisors_need_the_division():
    """Why exact_rdiv answers 0 for them: the product by the rounded reciprocal is another word for a good share of the operands."""
    g = _words(1 << 18, seed=19)
    with np.errstate(all="ignore"):
        for n in (3.0, 96.0, 100.0, 384.0, 768.0):
            share = _unequal(g * (np.float32(1.0) / np.float32(n)), g / np.float32(n)) / g.size
            print(n, "differs in %.3f of the words" % share)
            assert share > 0.1, (n, share)


def test_the_driver_is_clean_under_the_host_sanitizers(tmp_path):
    """The stand-alone driver, host side compiled with -fsanitize=address,undefined; it is its own program, nothing is preloaded."""
    exe = str(tmp_path / "update_rcp_driver_san")
    _build(exe, ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, env=env)
    assert p.returncode == 0 and DONE in p.stdout, p.stdout
