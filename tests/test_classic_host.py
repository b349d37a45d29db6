"""CPU tests of the log-MMSE baseline (include/bp_c_api.h): the float64 restatement in tests/classic_np.py
against known values, the fixture sentences of tests/test_classic_gpu.py against the conditions that make its comparisons fair,
and the argument checks of the library that come before any device use.

The conditions.  Every fixture sentence keeps min_t |vad_t - eta| >= 1e-3, so that the device's VAD decisions can be compared
with the restatement's without exemptions (a fixture that misses the margin gets another seed; the margin does not move).  Every
full-length sentence -- gated tones in white noise behind a noise-only lead, with or without an exact-zero gap -- also makes the
VAD take both outcomes, reaches the gamma cap and the xi floor and evaluates E1 on both sides of 1.  The edge sentences (one
sample, 200 samples, all zero) are too short or too empty for that; they are there for their own branches.  The wide sentences
(fea_dim 513 and 1025) that the GPU test holds to the restatement are vetted here too."""
import ctypes as C

import numpy as np
import pytest

import classic_np as CN

MARGIN = 1e-3
ALT = CN.ALT


# E1 to nine figures as the usual tables print it, and to sixteen (Abramowitz & Stegun table 5.1; E1(1) = 0.21938 39343 95520 27...).
# The bar is 1e-9 relative; it is taken against the sixteen-figure value because the nine-figure one is itself up to 5e-9 off
# (E1(1): 1.8e-9), and the nine figures are checked as printed.
@pytest.mark.parametrize("x,nine,want", [(0.5, 0.559773595, 0.5597735947761608), (1.0, 0.219383934, 0.2193839343955203),
                                         (2.0, 0.0489005107, 0.04890051070806112), (10.0, 4.15696893e-6, 4.156968929685324e-6)])
def test_e1_known_values(x, nine, want):
    got = CN.e1(x)[0]
    assert abs(got / want - 1.0) <= 1e-9
    assert float("%.9g" % got) == nine and float("%.9g" % want) == nine


def test_e1_branches_agree_across_one():
    for x in (1.0 - 1e-9, 1.0, 1.0 + 1e-9):
        a, b = CN.e1_series(np.array([x]))[0], CN.e1_cf(np.array([x]))[0]
        assert abs(a / b - 1.0) <= 1e-12, (x, a, b)
    assert CN.e1(1.0)[0] == CN.e1_series(np.array([1.0]))[0]    # x <= 1 is the series
    d = np.diff(CN.e1(np.array([0.999999, 1.0, 1.000001])))
    assert np.all(d < 0) and abs(d[0] / d[1] - 1.0) < 1e-5       # no step at the seam


@pytest.mark.parametrize("fea_dim", [33, 65, 129, 257])
def test_fixtures_are_fair(fea_dim):
    D, kinds, xs = [f for f in CN.fixtures() if f[0] == fea_dim][0]
    assert sorted(x.size for x in xs)[0] == 1 and len(xs) <= 6
    assert any(CN.n_frames(x.size, D) < CN.DEFAULTS["init_frames"] for x in xs)
    for i, (kind, x) in enumerate(zip(kinds, xs)):
        r = CN.reference(D, i)
        assert r["margin"] >= MARGIN, (kind, x.size, r["margin"])
        assert np.all(np.isfinite(r["G"])) and np.all(np.isfinite(r["vad"])) and np.all(np.isfinite(r["pcm"]))
        if kind in ("tones", "gap"):
            assert r["noise"].any() and not r["noise"].all(), (kind, x.size)
            assert r["cap"] and r["floor"] and r["v_le1"] and r["v_gt1"], (kind, x.size, r["cap"], r["floor"], r["v_le1"], r["v_gt1"])
            lead = int(CN.LEAD_HOPS * (D - 1))
            assert r["noise"][:6].all()                          # the lead is noise to the VAD
            assert np.sum(r["pcm"][:lead] ** 2) < np.sum(x[:lead].astype(np.float64) ** 2)   # ... and is turned down
        if kind == "gap":
            assert (r["G"] == 0.0).all(axis=1).any()             # whole frames with P = 0
        if D == 129:                                             # the non-default set runs on this call
            assert CN.reference(D, i, **ALT)["margin"] >= MARGIN, (kind, x.size)
    a, b = CN.reference(129, 0), CN.reference(129, 0, **ALT)
    assert not np.array_equal(a["noise"], b["noise"]) or np.abs(a["pcm"] - b["pcm"]).max() > 1.0


def test_wide_fixtures_are_fair():
    for D, xs in CN.wide_fixtures():
        r = CN.enhance(xs[0], D)
        assert r["margin"] >= MARGIN, (D, r["margin"])
        assert r["noise"].any() and not r["noise"].all() and r["v_le1"] and r["v_gt1"]
        assert xs[1].size == 1 and CN.n_frames(xs[2].size, D) >= CN.DEFAULTS["init_frames"]


def test_all_zero_sentence_gives_exact_zeros():
    r = CN.enhance(np.zeros(1500, np.float32), 129)
    assert np.all(r["pcm"] == 0.0) and np.all(r["G"] == 0.0) and not np.isnan(r["vad"]).any()
    assert np.allclose(r["vad"][0], -np.log(1.0 + CN.DEFAULTS["alpha"]))   # gamma = 0, xi = alpha at t = 0


def test_gain_of_a_pure_noise_frame_is_the_textbook_value():
    """One bin, gamma = 1, xi = alpha at t = 0: G = A exp(E1(A)/2) with A = alpha/(1+alpha)."""
    Y = np.full((1, 1), 3.0 + 4.0j)
    r = CN.recursion(Y, init_frames=1)
    A = 0.98 / 1.98
    assert r["G"][0, 0] == pytest.approx(A * np.exp(0.5 * CN.e1(A)[0]), rel=1e-14)
    assert r["vad"][0] == pytest.approx(A - np.log(1.98), rel=1e-14)


def test_overlap_add_inverts_the_analysis():
    x = np.random.default_rng(0).normal(0, 1000, 700)
    assert np.abs(CN.overlap_add(CN.analysis(x, 33), x.size) - x).max() < 1e-9


# ---- the library's checks that come before any device use (no GPU needed)
def _call(lib, pkg, fea_dim=129, lens=(10,), params=None, out=True):
    lens = np.array(lens, np.int32)
    x = np.zeros(max(int(lens.sum()), 1), np.float32)
    y = np.zeros_like(x)
    fp = C.POINTER(C.c_float)
    lm = pkg.logmmse_params(params)
    return lib.bp_logmmse_waves(0, fea_dim, None if lm is None else C.byref(lm), len(lens), lens.ctypes.data_as(C.POINTER(C.c_int)),
                                x.ctypes.data_as(fp), y.ctypes.data_as(fp) if out else None, None, None)


def test_defaults_and_symbols(pkg):
    lib = pkg.load_library()
    for s in ("bp_logmmse_defaults", "bp_logmmse_waves", "bp_eval_mix_logmmse"):
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS
    lm = pkg.BPLogmmseParams()
    assert lib.bp_logmmse_defaults(C.byref(lm)) == 0
    assert {k: getattr(lm, k) for k in CN.DEFAULTS} == CN.DEFAULTS
    assert lib.bp_logmmse_defaults(None) == -1


@pytest.mark.parametrize("bad", [{"alpha": 1.0}, {"alpha": -0.01}, {"alpha": float("nan")}, {"mu": 1.01}, {"mu": -0.01},
                                 {"eta": float("inf")}, {"eta": float("nan")}, {"xi_min_db": 0.5}, {"xi_min_db": -100.5},
                                 {"gamma_max": 0.99}, {"gamma_max": float("inf")}, {"init_frames": 0}])
def test_parameters_out_of_range_are_argument_errors(pkg, bad):
    lib = pkg.load_library()
    assert _call(lib, pkg, params=bad) == -1
    assert list(bad)[0] in lib.bp_last_error().decode()
    m = np.zeros(1, pkg.MIXTURE_DTYPE)
    s = np.zeros(3, np.float32)
    fp = C.POINTER(C.c_float)
    # (the parameters are checked before the handle is looked at: the message names the parameter, not the null handle)
    assert lib.bp_eval_mix_logmmse(None, C.byref(pkg.logmmse_params(bad)), 1, m.ctypes.data_as(C.c_void_p), 8000, s.ctypes.data_as(fp),
                                   s.ctypes.data_as(fp), None) == -1
    assert list(bad)[0] in lib.bp_last_error().decode()
    assert lib.bp_eval_mix_logmmse(None, None, 1, m.ctypes.data_as(C.c_void_p), 8000, s.ctypes.data_as(fp), s.ctypes.data_as(fp), None) == -1
    assert "null handle" in lib.bp_last_error().decode()


def test_bad_shapes_are_argument_errors(pkg):
    lib = pkg.load_library()
    assert _call(lib, pkg, fea_dim=100) == -1 and _call(lib, pkg, fea_dim=17) == -1 and _call(lib, pkg, fea_dim=2049) == -1
    assert _call(lib, pkg, lens=(10, 0)) == -1
    assert _call(lib, pkg, lens=()) == -1
    assert _call(lib, pkg, out=False) == -1
