"""Host tests of the dynamic noise-aware input (bp_set_nat): the float64 restatement in tests/dnat_np.py
against noise_np's tracker on its fixtures, what the rows do on noise that steps up, the wrong stagings that the GPU bar
(max|a - ref| / max|ref| < 1e-4, tests/util.py) would catch, the case table, and the argument rules of bp_set_nat that need no
device (a null handle is refused before anything is touched)."""
import itertools
import subprocess

import numpy as np
import pytest

import dnat_np as DN
import noise_np as NN
import wave_np as WN
from util import TOL, relerr


@pytest.mark.parametrize("D", [33, 129])
def test_restatement_reproduces_the_trackers_noise_rows(D):
    _, kinds, xs = NN.fixture(D)
    mean, istd = DN.norm(D)
    for i, kind in enumerate(kinds):
        ref = NN.reference(D, i)["noise"]
        Y = WN.analysis(xs[i], D)
        lam = DN.lambdas(Y)
        assert lam.shape == ref.shape
        assert relerr(lam, ref) < 1e-12, (D, kind)                # (two float64 analyses of the same samples)
        back = np.exp(DN.denormalise(DN.rows(Y, mean, istd), mean, istd))
        assert relerr(back, ref) < 1e-9, (D, kind)


@pytest.mark.parametrize("D", [33, 129])
def test_dynamic_rows_follow_a_step_and_the_static_row_does_not(D):
    _, kinds, xs = NN.fixture(D)
    x = xs[kinds.index("step")]
    mean, istd = DN.norm(D)
    Y = WN.analysis(x, D)
    dyn = np.exp(DN.denormalise(DN.rows(Y, mean, istd), mean, istd))
    level = NN.step_level_db(dyn, D)
    assert abs(level - NN.step_level_db(NN.recursion(Y, None, dict(mode=NN.MODE_SPP))["noise"], D)) < 1e-6
    assert level >= -2.5
    # the static row: the mean of the first 6 normalised frames, frozen at the early level (6 dB below the end)
    z = (WN.lps(Y) - mean) * istd
    stat = np.exp(DN.denormalise(np.repeat(WN.nat_row(z)[None, :], Y.shape[0], axis=0), mean, istd))
    assert NN.step_level_db(stat, D) <= -5.0


def test_wrong_stagings_miss_the_bar(record_property):
    """At every size the GPU test holds rows at (dnat_np.ALL_DIMS), on sentences of its frame classes; one factor per size and mutant."""
    for D in DN.ALL_DIMS:
        xs = DN.sentences(5, D)
        mean, istd = DN.norm(D)
        good = DN.blocks(xs, D, mean, istd)
        assert good.shape == (sum(DN.T_CLASSES), D)
        for m in DN.MUTANTS:
            bad = DN.blocks(xs, D, mean, istd, m)
            assert bad.shape == good.shape
            factor = relerr(bad, good) / TOL
            print("fea_dim %4d %-24s misses the bar by a factor of %.0f" % (D, m, factor))
            record_property("%s_%d" % (m, D), factor)
            assert factor > 10.0, (D, m, factor)


def test_case_table_has_no_empty_cell():
    have = {(c["mode"], c["entry"], c["fea_dim"], c["T"]) for c in DN.cases()}
    want = set(itertools.product(DN.MODES, DN.ENTRIES, DN.FEA_DIMS, DN.T_CLASSES))
    assert have == want and len(DN.cases()) == len(want)
    assert list(DN.ALL_DIMS) == [33, 65, 129, 257, 513, 1025] and [-(-D // 64) for D in DN.ALL_DIMS] == [1, 2, 3, 5, 9, 17]
    for D in DN.ALL_DIMS:
        assert [WN.n_frames(n, D) for n in DN.lengths(D)] == list(DN.T_CLASSES)
        assert max(DN.lengths(D)) <= 39 * (D - 1)                 # nothing longer than the 40-frame class
    assert min(DN.T_CLASSES) < 6 < max(DN.T_CLASSES) and 6 in DN.T_CLASSES and 7 in DN.T_CLASSES
    assert DN.WIDE % 64 == 1                                      # a last workgroup with one live lane


def test_selector_net_returns_the_block():
    D, ctx = 33, 3
    mean, istd = DN.norm(D)
    ls, W, b = DN.selector_net(D, ctx, mean, istd)
    rng = np.random.default_rng(0)
    x = rng.normal(size=(7, ls[0]))
    out = WN.forward(W, b, x)
    assert relerr(out, x[:, ctx * D:] / istd + mean) < 1e-6


def test_nat_key_is_checked_before_any_device_work(pkg):
    exe = {k: str(pkg.LIB_PATH).replace("libbp_hip.so", k) for k in ("bpenhance", "bpmix", "bpeval")}

    def run(tool, *args):
        r = subprocess.run([exe[tool]] + list(args), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr             # (the reference's convention: message on stdout, exit(0))
        return r.stdout

    assert "nat: sometimes is not static or dynamic" in run("bpenhance", "nat=sometimes")
    assert "bpmix: bad value for nat: sometimes" in run("bpmix", "nat=sometimes")
    assert "bpeval: bad value for nat: sometimes" in run("bpeval", "nat=sometimes")
    assert "method=logmmse takes no nat" in run("bpenhance", "method=logmmse", "fea_dim=129", "in_wav=a.wav", "out_wav=b.wav", "nat=dynamic")
    assert "pairs_list takes only" in run("bpeval", "pairs_list=p.list", "fea_dim=129", "nat=dynamic")


def test_set_nat_refuses_a_null_handle_without_a_device(pkg):
    lib = pkg.load_library()
    assert lib.bp_set_nat(None, pkg.NAT_DYNAMIC, None) != 0
    assert b"bp_set_nat" in lib.bp_last_error() and b"null handle" in lib.bp_last_error()
    assert pkg.NAT_MODES == {"static": 0, "dynamic": 1}
