"""CPU tests of the streaming contract: bp_stream_counts (host only, no device) against the restatement in tests/stream_np.py."""
import ctypes as C

import pytest

import stream_np as SN

CASES = [(1, 0), (7, 0), (7, 3), (7, 6)]


@pytest.mark.parametrize("fea_dim", [33, 129, 1025])
@pytest.mark.parametrize("ctx,toff", CASES)
@pytest.mark.parametrize("nat", [False, True])
def test_counts_match_restatement(pkg, fea_dim, ctx, toff, nat):
    hop = fea_dim - 1
    rs = range(0, 8 * hop + 2)
    for ended in (False, True):
        prev = (0, 0, 0)
        for r in rs:
            got = pkg.stream_counts(fea_dim, ctx, toff, nat, r, ended)
            assert got == SN.counts(fea_dim, ctx, toff, nat, r, ended), (r, ended)
            assert all(a >= b for a, b in zip(got, prev)), ("not monotone", r, ended)
            prev = got
            if ended:
                T = (r - 1) // hop + 2 if r else 0
                assert got == (T, T, r)
            else:
                assert got[2] <= max(0, r - hop) and got[1] <= got[0]


def test_ended_after_open_sentence_only_adds(pkg):
    """Closing a sentence never takes back what the open sentence had returned."""
    for fea_dim in (33, 129):
        for ctx, toff in CASES:
            for nat in (False, True):
                for r in range(1, 8 * (fea_dim - 1) + 2, 5):
                    a = pkg.stream_counts(fea_dim, ctx, toff, nat, r, False)
                    b = pkg.stream_counts(fea_dim, ctx, toff, nat, r, True)
                    assert all(y >= x for x, y in zip(a, b))


def test_counts_bad_arguments(pkg):
    bad = [dict(fea_dim=34), dict(fea_dim=17), dict(fea_dim=2049), dict(ctx=0), dict(toff=-1), dict(toff=7), dict(received=-1)]
    for kw in bad:
        a = dict(fea_dim=33, ctx=7, toff=3, received=10)
        a.update(kw)
        with pytest.raises(pkg.BPError, match="status -1"):
            pkg.stream_counts(a["fea_dim"], a["ctx"], a["toff"], True, a["received"], False)
    lib = pkg.load_library()
    v = C.c_int64()
    assert lib.bp_stream_counts(33, 7, 3, 1, 10, 0, None, C.byref(v), C.byref(v)) == -1
    assert lib.bp_stream_counts(33, 7, 3, 1, 10, 0, C.byref(v), C.byref(v), None) == -1


def test_stream_symbols_exported(pkg):
    lib = pkg.load_library()
    for s in ("bp_stream_open", "bp_stream_push", "bp_stream_close", "bp_stream_counts"):
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS
