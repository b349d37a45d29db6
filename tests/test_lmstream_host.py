"""CPU tests of the log-MMSE streams (bp_lmstream_*, include/bp_c_api.h): the counts against their
restatement in tests/lmstream_np.py, the properties that follow from the definition, and the argument checks that come before
any device use."""
import ctypes as C

import pytest

import lmstream_np as LN

SYMBOLS = ["bp_lmstream_open", "bp_lmstream_push", "bp_lmstream_close", "bp_lmstream_counts"]
CASES = [(D, init) for D in (33, 129) for init in (1, 4, 6)]


def _lib_counts(lib, fea_dim, init, received, ended, out=None):
    a, b, c = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    p = [C.byref(a), C.byref(b), C.byref(c)] if out is None else out
    rc = lib.bp_lmstream_counts(fea_dim, init, received, 1 if ended else 0, *p)
    return rc, (a.value, b.value, c.value)


@pytest.mark.parametrize("fea_dim,init", CASES)
def test_counts_equal_the_restatement(pkg, fea_dim, init):
    lib = pkg.load_library()
    hop = fea_dim - 1
    for ended in (False, True):
        for r in range((init + 3) * hop + 2):
            rc, got = _lib_counts(lib, fea_dim, init, r, ended)
            assert rc == 0 and got == LN.counts(fea_dim, init, r, ended), (r, ended, got)
            assert pkg.logmmse_stream_counts(fea_dim, init, r, ended) == got


@pytest.mark.parametrize("fea_dim,init", CASES)
def test_derived_properties(pkg, fea_dim, init):
    """From the definition: samples_out = max(0, frames_out - 1) hop with frames_out = 0 or received / hop never decreases with
    received; an ended sentence has returned all it received; frames_out is 0 exactly while the noise start is unknown, that is
    while frames_in < init_frames and the sentence has not ended (received > 0: nothing received has no frames either way)."""
    lib = pkg.load_library()
    hop = fea_dim - 1
    for f in (LN.counts, lambda *a: _lib_counts(lib, *a)[1]):
        last = 0
        for r in range((init + 3) * hop + 2):
            fi, fo, so = f(fea_dim, init, r, False)
            assert so >= last
            last = so
            fe, foe, soe = f(fea_dim, init, r, True)
            assert soe == r
            if r > 0:
                assert (fo == 0) == (fi < init) and foe > 0
                assert fo in (0, fi) and foe == fe == (r - 1) // hop + 2
            else:
                assert (fi, fo, so) == (0, 0, 0) == (fe, foe, soe)


def test_counts_bad_arguments(pkg):
    lib = pkg.load_library()
    assert _lib_counts(lib, 33, 6, -1, False)[0] == -1
    assert _lib_counts(lib, 100, 6, 10, False)[0] == -1
    assert _lib_counts(lib, 33, 0, 10, False)[0] == -1
    a = C.c_int64()
    for k in range(3):
        out = [C.byref(a)] * 3
        out[k] = None
        assert _lib_counts(lib, 33, 6, 10, False, out)[0] == -1
    assert b"bp_lmstream_counts" in lib.bp_last_error()
    with pytest.raises(pkg.BPError, match="status -1"):
        pkg.logmmse_stream_counts(33, 6, -1, False)


def test_symbols(pkg):
    lib = pkg.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS, s
    assert lib.bp_abi_version() == 5


@pytest.mark.parametrize("kw", [dict(params=dict(alpha=1.0)), dict(params=dict(init_frames=0)), dict(fea_dim=2049), dict(n_chan=0),
                                dict(n_chan=65537), dict(max_push_samples=0)])
def test_open_checks_come_before_the_device(pkg, kw):
    """BP_ERR_ARG whether or not the machine has a GPU: the checks come before hipGetDeviceCount."""
    args = dict(device=0, fea_dim=129, params=None, n_chan=1, max_push_samples=160)
    args.update(kw)
    with pytest.raises(pkg.BPError, match="bp_lmstream_open.*status -1"):
        pkg.logmmse_stream_open(**args)
    lib = pkg.load_library()
    lm = pkg.logmmse_params(args["params"])
    rc = lib.bp_lmstream_open(0, args["fea_dim"], None if lm is None else C.byref(lm), args["n_chan"], args["max_push_samples"], None)
    assert rc == -1                                              # (and before the null output pointer is looked at)
    assert lib.bp_lmstream_close(None) == 0
