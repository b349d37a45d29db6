"""Host tests of the post-processing of the LPS estimate (include/bp_c_api.h; no GPU): bp_gv_factors and
bp_post_defaults through the library against the restatement in tests/post_np.py, the equalisation property of the restatement,
and six wrong forms that each differ from it.

The equalisation bars (1e-5 relative): after the per-bin factors the variance of the post-processed rows is the clean variance up to
the fp32 rounding of each row value (2^-24 relative, averaging out over 600 frames) and of the factor itself (2^-24 relative, twice in
the variance: 1.2e-7); measured 1.0e-7 per bin after the per-bin factors and 4.4e-9 for the pooled figure after the single factor.
The bar leaves about 100x of margin over the larger."""
import ctypes as C

import numpy as np
import pytest

import post_np as PN

N, D = 600, 33


@pytest.fixture(scope="module")
def lib(pkg):
    import os
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return pkg.load_library()


def _data(seed=1):
    """clean LPS rows, and an over-smoothed estimate of them: half the deviation about the clean mean, plus a little noise"""
    rng = np.random.default_rng(seed)
    mean = rng.normal(8.0, 2.0, D)
    dev = rng.uniform(1.0, 3.0, D)
    ref = (mean + dev * rng.standard_normal((N, D))).astype(np.float32)
    est = (mean + 0.5 * (ref - mean) + 0.1 * rng.standard_normal((N, D))).astype(np.float32)
    return est, ref


def _var(v):
    s1, s2 = PN.part_sums(v)
    n = float(v.shape[0])
    return s2 / n - (s1 / n) ** 2


@pytest.mark.parametrize("mode", ["indep", "dep"])
def test_gv_factors_equal_the_restatement(pkg, lib, mode):
    est, ref = _data()
    st = PN.gv_sums(est, ref)
    c, s = pkg.gv_factors(st, mode)
    wc, ws = PN.gv_factors(st, mode)
    assert c.dtype == np.float32 and s.dtype == np.float32 and c.shape == (D,) and s.shape == (D,)
    assert np.array_equal(c.view(np.uint32), wc.view(np.uint32))
    assert np.array_equal(s.view(np.uint32), ws.view(np.uint32))
    if mode == "indep":
        assert np.all(s == s[0])
    else:
        assert len(set(s.tolist())) > 1
    assert np.all(s > 1.5) and np.all(s < 2.1)            # the estimate has about half the clean deviation


def test_gv_factors_errors(pkg, lib):
    est, ref = _data()
    st = PN.gv_sums(est, ref)
    with pytest.raises(pkg.BPError, match="status -1"):
        pkg.gv_factors(dict(st, frames=1))
    with pytest.raises(pkg.BPError, match="mode"):
        pkg.gv_factors(st, "both")
    flat = dict(st)
    flat["est_sq"] = st["est_sq"].copy()
    flat["est_sq"][7] = 0.5 * st["est_sum"][7] ** 2 / N  # a negative variance in bin 7
    with pytest.raises(pkg.BPError, match="bin 7"):
        pkg.gv_factors(flat)
    flat = dict(st)
    flat["ref_sq"] = st["ref_sq"].copy()
    flat["ref_sq"][30] = 0.0                              # ... and in bin 30 of the reference
    with pytest.raises(pkg.BPError, match="bin 30"):
        pkg.gv_factors(flat, "dep")
    const = PN.gv_sums(np.full((N, D), 2.0, np.float32), ref)           # a constant estimate: variance exactly 0
    with pytest.raises(pkg.BPError, match="bin 0"):
        pkg.gv_factors(const)
    dp = C.POINTER(C.c_double)
    a = [st[k].ctypes.data_as(dp) for k in ("est_sum", "est_sq", "ref_sum", "ref_sq")]
    out = np.zeros(D, np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.bp_gv_factors(34, N, *a, 0, fp, fp) == -1                      # 2 (fea_dim - 1) is no power of two
    assert lib.bp_gv_factors(D, N, *a, 2, fp, fp) == -1                       # no such mode
    assert lib.bp_gv_factors(D, N, a[0], None, a[2], a[3], 0, fp, fp) == -1   # a null pointer
    assert lib.bp_gv_factors(D, N, *a, 0, fp, None) == -1


def test_post_defaults(pkg, lib):
    p = pkg.BPPostParams()
    p.gv, p.mask_col, p.mask_lo, p.mask_hi, p.mask_weight = 7, 5, 0.1, 0.2, 0.3
    assert lib.bp_post_defaults(C.byref(p)) == 0
    assert (p.gv, p.mask_col, p.mask_lo, p.mask_hi, p.mask_weight) == (0, -1, 0.5, 0.5, 1.0)
    assert not p.gv_center and not p.gv_scale
    assert lib.bp_post_defaults(None) == -1
    assert lib.bp_abi_version() == 5
    with pytest.raises(pkg.BPError, match="come together"):
        pkg.post_params(gv_center=np.zeros(D, np.float32))


def test_equalisation_property():
    est, ref = _data(2)
    st = PN.gv_sums(est, ref)
    vr = _var(ref)
    c, s = PN.gv_factors(st, "dep")
    v = _var(PN.post(est, center=c, scale=s))
    err_dep = float(np.abs(v / vr - 1.0).max())
    assert err_dep <= 1e-5, err_dep
    c, s = PN.gv_factors(st, "indep")
    v = _var(PN.post(est, center=c, scale=s))
    err_indep = abs(D / float(np.sum(v / vr)) - 1.0)
    assert err_indep <= 1e-5, err_indep
    # and it was needed: the raw estimate has about a quarter of the clean variance
    assert np.all(_var(est) / vr < 0.35)


def test_wrong_forms_differ_from_the_restatement():
    est, ref = _data(3)
    rng = np.random.default_rng(4)
    y = (ref + rng.normal(2.0, 1.0, ref.shape)).astype(np.float32)
    m = rng.uniform(0.0, 1.0, ref.shape).astype(np.float32)
    st = PN.gv_sums(est, ref)
    c, s = PN.gv_factors(st, "dep")
    lo, hi, w = 0.3, 0.8, 0.6
    want = PN.post(est, y, m, c, s, lo, hi, w)
    f32 = np.float32

    def differs(got):
        return int((np.asarray(got, f32).view(np.uint32) != want.view(np.uint32)).sum()) >= 1

    # gate before GV
    g = PN.post(PN.post(est, y, m, None, None, lo, hi, w), center=c, scale=s)
    assert differs(g)
    # scale about zero
    assert differs(PN.post(est, y, m, np.zeros(D, f32), s, lo, hi, w))
    # scale about the estimate's mean
    assert differs(PN.post(est, y, m, (st["est_sum"] / N).astype(f32), s, lo, hi, w))
    # lo and hi swapped (the ramp runs the other way: taken as written, hi < lo is the step at hi)
    assert differs(PN.post(est, y, m, c, s, hi, lo, w))
    # weight ignored
    assert differs(PN.post(est, y, m, c, s, lo, hi, 1.0))
    # beta as the mean of the per-bin factors
    ci, si = PN.gv_factors(st, "indep")
    wrong = np.full(D, f32(np.mean(s.astype(np.float64))), f32)
    a, b = PN.post(est, center=ci, scale=si), PN.post(est, center=ci, scale=wrong)
    assert si[0] != wrong[0] and int((a.view(np.uint32) != b.view(np.uint32)).sum()) >= 1


def test_gate_edges():
    f32 = np.float32
    m = np.array([[0.0, 0.3, 0.55, 0.8, 1.0, np.nan, 0.79999995, 0.30000004]], f32)
    u = PN.gate(m, 0.3, 0.8)
    assert u[0, 0] == 0 and u[0, 1] == 0 and 0 < u[0, 2] < 1 and u[0, 3] == 1 and u[0, 4] == 1 and u[0, 5] == 0
    assert 0 < u[0, 6] <= 1 and 0 < u[0, 7] < 1
    s = PN.gate(m, 0.5, 0.5)
    assert s.tolist() == [[0, 0, 1, 1, 1, 0, 1, 0]]
    x = np.full((1, 8), 3.0, f32)
    y = np.full((1, 8), np.log(1e-10), f32)               # the noisy LPS at its floor
    out = PN.post(x, y, m, lo=0.5, hi=0.5, weight=1.0)
    assert np.array_equal(out[0, [2, 3, 4, 6]], y[0, [2, 3, 4, 6]]) and np.all(out[0, [0, 1, 5, 7]] == 3.0)
